// comb_core.hpp — the per-packet combiner's state machine, independent of the device: engine.cpp
// instantiates it over HIP (HipComb), tests/sanitize/comb_test.cpp (ASan/UBSan and TSan builds) over
// a fake device whose launches the test holds and releases.
//
// Per-packet AES-256-GCM calls (neb_encrypt_danger / neb_decrypt_danger) that arrive while
// max_inflight launches are in flight join one pinned batch of up to kCombMax requests, which its
// first request (the leader) launches as a whole (gcm_one_batch_kernel) as soon as one of the
// launches ahead completes; the leader polls every status, wakes the others, and each copies its
// own result out. A call that finds a launch free launches alone (Dev::solo: the packet in the
// kernel arguments), so up to max_inflight threads see no change; past that the batches grow with
// the offered load. ChaCha20-Poly1305 calls (its batch kernel's statuses carry no release of the
// payload before them) and calls too large for a slot always go alone.
//
// The steps (take, join, lead, collect) serve both call(), the path of the C ABI's per-packet
// calls, and run(), which places n requests of one thread in one batch in the given order
// (neb_engine_pkt_launch, for tests: request r is slot r).
//
// Dev has: Buf (bytes of pinned, mapped memory: operator uint8_t*), Token (a launch's completion
// handle), Guard (constructed from the Dev for the span of a call's device work),
//   bool reserve(Buf&, size_t bytes)            allocate a batch's buffer (false: the error is set)
//   int  solo(const CombReq&, int32_t* st)      the call alone, to completion: NEB_OK or an error
//   bool launch(int open, const neb_desc*, int32_t* status, uint8_t* slots, uint32_t n,
//               uint32_t turn, Token&)          asynchronous; `turn` counts the combined launches
//   bool poll(Token&, const int32_t* p)         p's status word published (!= -1) within the poll time
//   bool sync(Token&)                           wait for the launch (false: it failed, the error is set)
//   void count(uint32_t n)                      n per-packet calls went out combined (neb_engine_stats)
#pragma once

#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/nebula_aead.h"
#include "host_common.hpp"

namespace neb {

// One per-packet call: `in` is the plaintext (seal) or ciphertext + tag (open), pay_len the
// payload's length without the tag, dst takes pay_len + 16 (seal) or pay_len (open) bytes.
struct CombReq {
    int alg = 0, open = 0;
    uint32_t key_id = 0;
    uint64_t n = 0;  // the counter
    const uint8_t* ad = nullptr;
    size_t ad_len = 0;
    const uint8_t* in = nullptr;
    size_t in_len = 0, pay_len = 0;
    uint8_t* dst = nullptr;
};

inline size_t comb_pay(size_t ad_len) { return (ad_len + 15) & ~(size_t)15; }  // the payload's place in a slot

// A call the combiner may put into a batch: AES-256-GCM, its AAD (padded to 16) and input within
// kOneBytes (what the alone kernel's argument block holds), and the result within the slot.
inline bool comb_fits(const CombReq& q) {
    if (q.alg != NEB_ALG_AESGCM || q.ad_len > kOneBytes || q.in_len > kOneBytes || q.pay_len > kOneBytes) return false;
    const size_t pay = comb_pay(q.ad_len);
    return pay + std::max(q.in_len, q.pay_len + 16) <= kCombSlot && pay + q.in_len <= kOneBytes;
}

// A per-packet call's result from its slot into the caller's buffer, by status: a sealed or opened
// packet is copied; a failed open leaves zeros (the kernel's in-place zeroing, written here so the
// slot is never read); any other status (no key, exhausted counter) writes nothing, as the
// reference returns before touching out (aesgcm.go:28-30). The slot's bytes are read only when the
// kernel wrote them: slots are shared by every thread and cipher of the engine, so anything else
// there is another call's packet.
inline void copy_result(int open, int32_t st, uint8_t* dst, const uint8_t* slot, size_t pay_len) {
    const size_t out_len = open ? pay_len : pay_len + 16;
    if (!out_len) return;
    if (st == NEB_STATUS_OK)
        std::memcpy(dst, slot, out_len);
    else if (open && st == NEB_STATUS_AUTH_FAILED)
        std::memset(dst, 0, out_len);
}

// A batch's buffer: descriptors | statuses | slots (request r's bytes in slot r, kCombSlot apart)
constexpr size_t kCombDescOff = 0, kCombStatusOff = 2u << 10, kCombSlotsOff = 4u << 10;  // 2 KiB for each
static_assert(kCombMax * sizeof(neb_desc) <= kCombStatusOff && kCombMax * 4u <= kCombSlotsOff - kCombStatusOff, "");
constexpr size_t kCombBytes = kCombSlotsOff + (size_t)kCombMax * kCombSlot;

template <class Dev>
struct CombBatch {
    typename Dev::Buf h;  // mapped: descriptors | statuses | slots
    uint32_t n = 0;       // requests joined
    int open = 0;
    bool launched = false, idle = true;  // (CombCore::mu_) idle: on the free list
    typename Dev::Token tok{};
    std::atomic<uint32_t> left{0};  // requests whose owner has not copied its result out yet
    // The leader saw every status: the owners may copy out. A futex word of the batch's own, so the
    // owners wake without queueing on a mutex (64 threads on a 16-CPU share: p99 23 ms when they
    // woke through the combiner's mutex).
    std::atomic<uint32_t> done{0};
    bool failed = false;  // written before done's release
    void finish(bool f) {
        failed = f;
        done.store(1, std::memory_order_release);
        syscall(SYS_futex, reinterpret_cast<uint32_t*>(&done), FUTEX_WAKE_PRIVATE, INT_MAX, nullptr, nullptr, 0);
    }
    bool wait() {  // the failure flag
        while (!done.load(std::memory_order_acquire))
            syscall(SYS_futex, reinterpret_cast<uint32_t*>(&done), FUTEX_WAIT_PRIVATE, 0, nullptr, nullptr, 0);
        return failed;
    }
    neb_desc* desc() const { return reinterpret_cast<neb_desc*>(h + kCombDescOff); }
    int32_t* status() const { return reinterpret_cast<int32_t*>(h + kCombStatusOff); }
    uint8_t* slots() const { return h + kCombSlotsOff; }
};

template <class Dev>
class CombCore {
  public:
    using Batch = CombBatch<Dev>;
    Dev dev;

    // max_inflight: launches (alone or combined) in flight before calls combine; max_solo: of them
    // alone (the device's slots for alone calls)
    CombCore(uint32_t max_inflight, uint32_t max_solo) : max_inflight_(max_inflight), max_solo_(max_solo) {}
    CombCore(const CombCore&) = delete;
    CombCore& operator=(const CombCore&) = delete;

    // One per-packet call: alone while a launch slot is free and no batch is gathering, else as a
    // request of the batch the next completed launch frees a slot for. NEB_OK: *st_out is the
    // packet's status and dst holds the result (copy_result).
    int call(const CombReq& q, int32_t* st_out) {
        if (!comb_fits(q)) return dev.solo(q, st_out);
        std::unique_lock<std::mutex> lk(mu_);
        Batch*& ob = open_[q.open ? 1 : 0];
        // Alone while a launch and a slot for alone calls are free and no batch is gathering
        if (inflight_ < max_inflight_ && solo_ < max_solo_ && !ob) {
            inflight_++;
            solo_++;
            lk.unlock();
            const int rc = dev.solo(q, st_out);
            lk.lock();
            inflight_--;
            solo_--;
            lk.unlock();
            launch_cv_.notify_all();
            return rc;
        }
        typename Dev::Guard dg(dev);
        if (!ob) {
            int rc = NEB_OK;
            ob = take(q.open, &rc);
            if (!ob) return rc;
        }
        Batch* b = ob;
        const uint32_t i = join(b, q);
        if (b->n == kCombMax) ob = nullptr;  // full: the next call starts another
        // The batch's first request leads it: it waits until a launch completes, launches the batch as
        // it stands then (every joined request is filled: joiners fill under the mutex), polls every
        // status and wakes the others. Under load the batch gathers for as long as the launches ahead
        // of it run, so its size follows the offered load; one thread spins per launch, the rest sleep
        // (64 threads spinning on a 16-CPU share starved the launches: p99 37 ms).
        if (i == 0) lead(lk, b);
        else lk.unlock();
        return collect(b, i, q, st_out);
    }

    // n <= kCombMax requests of one direction, each one comb_fits, as one batch of their own in the
    // given order (request r in slot r), launched as a leader launches its batch: the batch comes
    // from the free list, never the gathering one, and waits for a launch slot like any other.
    // st[r] and q[r].dst as call() leaves them. NEB_ERR_INVALID: nothing was launched or written.
    int run(int open, const CombReq* q, uint32_t n, int32_t* st) {
        if (n > kCombMax || (n && (!q || !st))) return NEB_ERR_INVALID;
        for (uint32_t r = 0; r < n; r++)
            if (!comb_fits(q[r]) || (q[r].open != 0) != (open != 0)) return NEB_ERR_INVALID;
        if (n == 0) return NEB_OK;
        std::unique_lock<std::mutex> lk(mu_);
        typename Dev::Guard dg(dev);
        int rc = NEB_OK;
        Batch* b = take(open, &rc);
        if (!b) return rc;
        for (uint32_t r = 0; r < n; r++) join(b, q[r]);
        lead(lk, b);
        for (uint32_t r = 0; r < n; r++) {
            const int rr = collect(b, r, q[r], st + r);
            if (rr != NEB_OK) rc = rr;
        }
        return rc;
    }

    // {launches of combined batches, calls they carried}
    void counters(uint64_t out[2]) const {
        out[0] = launches_.load(std::memory_order_relaxed);
        out[1] = combined_.load(std::memory_order_relaxed);
    }

    // The accounting at one instant (tests, diagnostics)
    struct State {
        uint32_t inflight, solo;
        uint32_t batches, free_batches;  // buffers allocated, and those of them on the free list
        uint32_t open_n[2];              // requests in the gathering batch of [seal, open] (0: none)
        uint32_t gathering;              // requests joined to batches not yet launched
    };
    State state() {
        std::lock_guard<std::mutex> g(mu_);
        State s{inflight_, solo_, (uint32_t)all_.size(), (uint32_t)free_.size(), {0, 0}, 0};
        for (int k = 0; k < 2; k++) s.open_n[k] = open_[k] ? open_[k]->n : 0;
        for (auto& b : all_)
            if (!b->idle && !b->launched) s.gathering += b->n;
        return s;
    }

  private:
    // A batch off the free list (a new one when that is empty), empty and not yet launched. (mu_)
    Batch* take(int open, int* rc) {
        if (free_.empty()) {
            std::unique_ptr<Batch> nb(new (std::nothrow) Batch);
            if (!nb) {
                *rc = NEB_ERR_INVALID;
                return nullptr;
            }
            if (!dev.reserve(nb->h, kCombBytes)) {
                *rc = NEB_ERR_HIP;
                return nullptr;
            }
            free_.push_back(nb.get());
            all_.push_back(std::move(nb));
        }
        Batch* b = free_.back();
        free_.pop_back();
        b->n = 0;
        b->launched = false;
        b->idle = false;
        b->failed = false;
        b->done.store(0, std::memory_order_relaxed);
        b->open = open ? 1 : 0;
        return b;
    }

    // q into b's next slot: its bytes, its descriptor (offsets from the slots' base, in place in the
    // slot), its status word unpublished. The slot's index. (mu_)
    uint32_t join(Batch* b, const CombReq& q) {
        const uint32_t i = b->n++;
        const size_t pay = comb_pay(q.ad_len);
        uint8_t* slot = b->slots() + (size_t)i * kCombSlot;
        if (q.ad_len) std::memcpy(slot, q.ad, q.ad_len);
        if (q.in_len) std::memcpy(slot + pay, q.in, q.in_len);
        neb_desc& d = b->desc()[i];
        d = neb_desc{};
        d.aad_off = (uint64_t)i * kCombSlot;
        d.src_off = d.dst_off = d.aad_off + pay;
        d.counter = q.n;
        d.len = (uint32_t)q.pay_len;
        d.aad_len = (uint32_t)q.ad_len;
        d.key_id = q.key_id;
        __atomic_store_n(b->status() + i, -1, __ATOMIC_RELAXED);
        return i;
    }

    // The leader's part: wait for a launch slot, close the batch, launch it, see every status (or
    // wait for the launch when one does not come), give the launch slot back and wake the owners.
    // Called with lk held; returns with it released.
    void lead(std::unique_lock<std::mutex>& lk, Batch* b) {
        launch_cv_.wait(lk, [&] { return inflight_ < max_inflight_; });
        inflight_++;
        if (open_[b->open] == b) open_[b->open] = nullptr;
        b->launched = true;
        b->left.store(b->n, std::memory_order_relaxed);
        const uint32_t turn = next_++;
        const uint32_t cnt = b->n;
        dev.count(cnt);
        lk.unlock();
        bool ok = dev.launch(b->open, b->desc(), b->status(), b->slots(), cnt, turn, b->tok);
        launches_.fetch_add(1, std::memory_order_relaxed);
        combined_.fetch_add(cnt, std::memory_order_relaxed);
        if (ok) {
            bool slow = false;
            for (uint32_t k = 0; k < cnt && !slow; k++) slow = !dev.poll(b->tok, b->status() + k);
            if (slow) ok = dev.sync(b->tok);  // a slow device: the launch's completion says when
        }
        lk.lock();
        inflight_--;
        lk.unlock();
        launch_cv_.notify_all();
        b->finish(!ok);
    }

    // Request i's owner: sleep until the leader has seen the statuses, copy the result out, and, as
    // the last owner out, put the batch back on the free list.
    // (the owners sleep rather than poll their own status words: 8 spinners measured 317-336 k /
    // 363-387 k calls/s at 16 / 32 threads against 338-341 k / 530-542 k sleeping)
    int collect(Batch* b, uint32_t i, const CombReq& q, int32_t* st_out) {
        const bool failed = b->wait();
        const int32_t st = failed ? -1 : __atomic_load_n(b->status() + i, __ATOMIC_ACQUIRE);
        if (st != -1) copy_result(q.open, st, q.dst, b->slots() + (size_t)i * kCombSlot + comb_pay(q.ad_len), q.pay_len);
        if (b->left.fetch_sub(1, std::memory_order_acq_rel) == 1) {
            std::lock_guard<std::mutex> g(mu_);
            b->idle = true;
            free_.push_back(b);
        }
        if (st == -1) return NEB_ERR_HIP;
        *st_out = st;
        return NEB_OK;
    }

    const uint32_t max_inflight_, max_solo_;
    std::mutex mu_;
    uint32_t inflight_ = 0;  // launches (alone or combined) not yet complete, at most max_inflight_
    uint32_t solo_ = 0;      // of them alone, at most max_solo_
    std::condition_variable launch_cv_;  // a launch completed (the leaders of gathering batches wait)
    Batch* open_[2] = {};                // accepting requests: [seal / open]
    std::vector<Batch*> free_;
    std::vector<std::unique_ptr<Batch>> all_;
    uint32_t next_ = 0;  // combined launches so far (the device spreads them over its streams)
    std::atomic<uint64_t> launches_{0}, combined_{0};
};

}  // namespace neb
