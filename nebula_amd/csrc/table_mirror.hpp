// table_mirror.hpp — the device copy of a lookup table whose host copy is authoritative (the index
// table, index.cpp; the TX table, route.cpp): two images of Slot in device memory, the active one
// brought up to date by the table's scatter kernel on the caller's stream, the spare one taking the
// next rebuild. It knows nothing of what a slot or an op means; it keeps the order of the device work:
//   - a stream reads the image that is active when its launch is enqueued (read), and the image's
//     list of (stream, event) uses remembers the last work every stream has on it;
//   - the spare image is overwritten only after the host has waited for all of its uses (rebuild),
//     and becomes the active one only once its upload has completed;
//   - a pinned staging buffer is refilled only after the host has waited for the launch that read it;
//   - an update's `first` ops are all launched before any of its `second` ops (the owner puts new
//     records in the first list and the tombstones of older ones in the second, so a replaced key is
//     never absent);
//   - updates given on different streams take effect in the order of the calls (update_ev);
//   - drain() waits for every event, after which the owner may delete the mirror.
// The owner serialises init, update, rebuild and drain (its own lock, taken outside this one); read
// and lock() may come from any thread. Host-only logic over a device policy, like workspace.hpp: the
// tables bind it to HipWsApi, tests/sanitize/mirror_test.cpp to a fake that logs the calls. Beyond
// workspace.hpp's members Api has memset, copy_h2d, stream_sync, device_sync, event_create_host and
// kPinned. Returns NEB_OK, NEB_ERR_HIP for a failed device call, NEB_ERR_INVALID out of memory.
#pragma once

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/nebula_aead.h"
#include "workspace.hpp"  // (and hip_owned.hpp)

namespace neb {

// A word of the host copy, for the searches that also run on a device image (device_common.hpp,
// LoadAgent).
struct HostLoad {
    uint64_t operator()(const uint64_t* p) const { return *p; }
};

constexpr uint32_t kStageOps = 4096;  // ops per scatter launch (two pinned staging buffers)

#define NEB_MIRROR_TRY(x)                         \
    do {                                          \
        if ((x) != Api::kOk) return NEB_ERR_HIP;  \
    } while (0)

template <class Api, class Slot, class Op>
class TableMirror {
  public:
    using Stream = typename Api::Stream;
    using Event = typename Api::Event;
    TableMirror() = default;
    TableMirror(const TableMirror&) = delete;
    TableMirror& operator=(const TableMirror&) = delete;
    ~TableMirror() {  // after drain(), with the owner's device current
        for (auto& us : uses_)
            for (Use& u : us) Api::event_destroy(u.ev);
        for (Event ev : {stage_ev_[0], stage_ev_[1], update_ev_})
            if (ev) Api::event_destroy(ev);
    }

    // Both images zeroed before any stream can read them. After a failure: drain() and delete.
    int init(size_t nslots) {
        bytes_ = nslots * sizeof(Slot);
        for (int k = 0; k < 2; k++) {
            NEB_MIRROR_TRY(image_[k].reserve(bytes_));
            NEB_MIRROR_TRY(Api::memset(image_[k], 0, bytes_));
            NEB_MIRROR_TRY(stage_[k].reserve(kStageOps * sizeof(Op)));
            NEB_MIRROR_TRY(Api::event_create_host(&stage_ev_[k]));
        }
        NEB_MIRROR_TRY(upload_.reserve(bytes_));
        NEB_MIRROR_TRY(Api::event_create_host(&update_ev_));
        NEB_MIRROR_TRY(Api::device_sync());
        return NEB_OK;
    }

    // first, then second, to the active image on s. scatter(image, ops, n, s) is the table's launcher.
    template <class Scatter>
    int update(const std::vector<Op>& first, const std::vector<Op>& second, Stream s, Scatter scatter) {
        if (first.empty() && second.empty()) return NEB_OK;
        std::lock_guard<std::mutex> g(dmu_);
        if (update_pending_ && update_stream_ != s) NEB_MIRROR_TRY(Api::stream_wait(s, update_ev_));
        for (const std::vector<Op>* ops : {&first, &second})
            for (size_t at = 0; at < ops->size(); at += kStageOps) {
                const uint32_t cnt = (uint32_t)std::min<size_t>(kStageOps, ops->size() - at);
                const int k = stage_next_;
                stage_next_ ^= 1;
                if (stage_busy_[k]) NEB_MIRROR_TRY(Api::event_sync(stage_ev_[k]));  // its last launch has read it
                std::memcpy(stage_[k], ops->data() + at, (size_t)cnt * sizeof(Op));
                NEB_MIRROR_TRY(scatter((Slot*)image_[active_], (const Op*)stage_[k], cnt, s));
                NEB_MIRROR_TRY(Api::event_record(stage_ev_[k], s));
                stage_busy_[k] = true;
            }
        NEB_MIRROR_TRY(Api::event_record(update_ev_, s));
        update_stream_ = s;
        update_pending_ = true;
        return note_use(active_, s);
    }

    // slots (the whole rebuilt host copy) into the spare image, then the switch. extra(spare, s)
    // enqueues whatever else travels with an image; on_switch(spare) runs under the lock, with the
    // switch. Blocks: for the spare image's users, then for s.
    template <class Extra, class OnSwitch>
    int rebuild(const Slot* slots, Stream s, Extra extra, OnSwitch on_switch) {
        int spare;
        {
            std::lock_guard<std::mutex> g(dmu_);
            spare = active_ ^ 1;
        }
        // nothing new can start on the spare image: its list stays as it is, reads note the active one
        for (const Use& u : uses_[spare]) NEB_MIRROR_TRY(Api::event_sync(u.ev));
        std::memcpy(upload_, slots, bytes_);
        NEB_MIRROR_TRY(Api::copy_h2d(image_[spare], upload_, bytes_, s));
        NEB_MIRROR_TRY(extra(spare, s));
        NEB_MIRROR_TRY(Api::stream_sync(s));  // complete before any stream can be pointed at it
        std::lock_guard<std::mutex> g(dmu_);
        active_ = spare;
        update_pending_ = false;  // later updates go to this image, which nothing else writes
        on_switch(spare);
        return NEB_OK;
    }
    int rebuild(const Slot* slots, Stream s) {
        return rebuild(slots, s, [](int, Stream) { return Api::kOk; }, [](int) {});
    }

    // launch(k, image) enqueues a reader of the active image on s; a rebuild into it waits for it.
    template <class Launch>
    int read(Stream s, Launch launch) const {
        std::lock_guard<std::mutex> g(dmu_);
        NEB_MIRROR_TRY(launch(active_, (const Slot*)image_[active_]));
        return note_use(active_, s);
    }

    void drain() {
        for (auto& us : uses_)
            for (Use& u : us) (void)Api::event_sync(u.ev);
        for (Event ev : {stage_ev_[0], stage_ev_[1], update_ev_})
            if (ev) (void)Api::event_sync(ev);
    }

    // The lock of read and of the switch, for what the owner keeps beside the images.
    std::mutex& lock() const { return dmu_; }

  private:
    struct Use {  // the last work a stream has enqueued on an image
        Stream s;
        Event ev;
    };
    // Record that stream s has work on image k in flight (dmu_ held).
    int note_use(int k, Stream s) const {
        for (Use& u : uses_[k])
            if (u.s == s) {
                NEB_MIRROR_TRY(Api::event_record(u.ev, s));
                return NEB_OK;
            }
        try {
            uses_[k].reserve(uses_[k].size() + 1);
        } catch (const std::bad_alloc&) {
            return NEB_ERR_INVALID;
        }
        Event ev{};
        NEB_MIRROR_TRY(Api::event_create_host(&ev));
        uses_[k].push_back(Use{s, ev});
        NEB_MIRROR_TRY(Api::event_record(ev, s));
        return NEB_OK;
    }

    mutable std::mutex dmu_;  // which image is active, and the events
    size_t bytes_ = 0;        // of one image
    OwnedBuf<Api, Slot> image_[2];
    int active_ = 0;
    mutable std::vector<Use> uses_[2];
    OwnedBuf<Api, Op, (int)Api::kPinned> stage_[2];
    Event stage_ev_[2] = {};
    bool stage_busy_[2] = {false, false};
    int stage_next_ = 0;
    OwnedBuf<Api, Slot, (int)Api::kPinned> upload_;  // a rebuilt image on its way to the device
    Event update_ev_{};
    Stream update_stream_{};
    bool update_pending_ = false;
};

#undef NEB_MIRROR_TRY

}  // namespace neb
