// mirror_test.cpp — sanitizer test (ASan + UBSan, and TSan) of the lookup tables' device-image
// protocol (nebula_amd/csrc/table_mirror.hpp) over a fake device written like workspace_test.cpp's:
// it logs every call, keeps each recorded event "pending" until the host has waited for it, hands
// out host memory as device memory, and can fail its k-th call. Its "scatter" applies the ops to the
// image at once, so an image can be compared with the host slots. The test pins, from the log, the
// six ordering rules the header lists. TEST INFRASTRUCTURE; `make -C tests/sanitize`.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <random>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../nebula_amd/csrc/table_mirror.hpp"

static int fails = 0;
#define CHECK(x)                                                                       \
    do {                                                                               \
        if (!(x)) {                                                                    \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
            fails++;                                                                   \
        }                                                                              \
    } while (0)

struct FakeEvent {
    int id = 0;
    bool pending = false;  // recorded, and the host has not waited for it since
};

using Log = std::vector<std::string>;

// Streams are small numbers; events are named e0, e1, ... in the order of their creation (init
// creates e0 and e1 for the staging buffers and e2 for the updates); device allocations i0, i1 are
// the images, pinned ones b0, b1 the staging buffers (b2: the upload buffer).
struct Fake {
    using Stream = int;
    using Event = FakeEvent*;
    using Error = int;
    static constexpr int kOk = 0;
    static constexpr unsigned kPinned = 0;

    static inline std::mutex mu;  // the fake's own state: the mirror calls it from several threads
    static inline Log log;
    static inline bool logging = true;
    static inline int fail_at = 0;  // the k-th call from now fails (0: none)
    static inline int next_event = 0;
    static inline std::set<FakeEvent*> events;
    static inline std::vector<uint8_t*> dev, pinned;  // live allocations, in order

    static int call(const std::string& what) {  // mu held
        if (logging) log.push_back(what);
        return fail_at && --fail_at == 0 ? 2 : kOk;
    }
    static std::string name(const std::vector<uint8_t*>& v, const void* p, char c) {
        for (size_t k = 0; k < v.size(); k++)
            if (v[k] == p) return c + std::to_string(k);
        return "?";
    }
    static void note(const std::string& what) {
        std::lock_guard<std::mutex> g(mu);
        if (logging) log.push_back(what);
    }
    static void reset() {
        log.clear();
        next_event = 0;
        fail_at = 0;
    }

    static int event_create_host(Event* ev) {
        std::lock_guard<std::mutex> g(mu);
        if (call("create:e" + std::to_string(next_event))) return 2;
        *ev = new FakeEvent{next_event++, false};
        events.insert(*ev);
        return kOk;
    }
    static int event_sync(Event ev) {
        std::lock_guard<std::mutex> g(mu);
        if (call("sync:e" + std::to_string(ev->id))) return 2;
        ev->pending = false;
        return kOk;
    }
    static int event_record(Event ev, Stream s) {
        std::lock_guard<std::mutex> g(mu);
        if (call("record:e" + std::to_string(ev->id) + ":s" + std::to_string(s))) return 2;
        ev->pending = true;
        return kOk;
    }
    static void event_destroy(Event ev) {
        std::lock_guard<std::mutex> g(mu);
        CHECK(!ev->pending);  // the owner drained first
        events.erase(ev);
        delete ev;
    }
    static int stream_wait(Stream s, Event ev) {
        std::lock_guard<std::mutex> g(mu);
        return call("wait:s" + std::to_string(s) + ":e" + std::to_string(ev->id));
    }
    static int stream_sync(Stream s) {
        std::lock_guard<std::mutex> g(mu);
        return call("ssync:s" + std::to_string(s));
    }
    static int device_sync() {
        std::lock_guard<std::mutex> g(mu);
        return call("dsync");
    }
    static int memset(void* p, int v, size_t bytes) {
        std::lock_guard<std::mutex> g(mu);
        if (call("memset:" + name(dev, p, 'i'))) return 2;
        std::memset(p, v, bytes);
        return kOk;
    }
    static int copy_h2d(void* dst, const void* src, size_t bytes, Stream s) {
        std::lock_guard<std::mutex> g(mu);
        if (call("copy:" + name(dev, dst, 'i') + ":" + name(pinned, src, 'b') + ":s" + std::to_string(s))) return 2;
        std::memcpy(dst, src, bytes);
        return kOk;
    }
    static int alloc(std::vector<uint8_t*>* v, const char* what, uint8_t** p, size_t bytes) {
        std::lock_guard<std::mutex> g(mu);
        if (call(what)) return 2;
        *p = static_cast<uint8_t*>(std::malloc(bytes));
        v->push_back(*p);
        return kOk;
    }
    static void release(std::vector<uint8_t*>* v, uint8_t* p) {
        std::lock_guard<std::mutex> g(mu);
        for (FakeEvent* ev : events) CHECK(!ev->pending);  // nothing is in flight when memory goes
        for (auto& q : *v)
            if (q == p) q = nullptr;
        while (!v->empty() && !v->back()) v->pop_back();
        std::free(p);
    }
    static int mem_alloc(uint8_t** p, size_t bytes) { return alloc(&dev, "alloc", p, bytes); }
    static void mem_free(uint8_t* p) { release(&dev, p); }
    static int host_alloc(uint8_t** p, size_t bytes, unsigned) { return alloc(&pinned, "halloc", p, bytes); }
    static void host_free(uint8_t* p) { release(&pinned, p); }
};

struct Slot {
    uint64_t v;
};
struct Op {
    uint32_t slot;
    uint32_t list;  // 1: handed over in `first`, 2: in `second`
    uint64_t v;
};
using Mirror = neb::TableMirror<Fake, Slot, Op>;
constexpr uint32_t kStage = neb::kStageOps;

static Log take() {
    std::lock_guard<std::mutex> g(Fake::mu);
    Log l;
    l.swap(Fake::log);
    return l;
}
static bool starts(const std::string& s, const char* p) { return s.rfind(p, 0) == 0; }
static size_t count(const Log& l, const char* prefix) {
    size_t n = 0;
    for (const std::string& c : l) n += starts(c, prefix);
    return n;
}

// The table's launcher: logs the staging buffer and the count, applies the ops at once, and checks
// that a launch is all of one list and that no `first` op comes after a `second` one.
static int last_list = 0;
static int scatter(Slot* image, const Op* ops, uint32_t n, int s) {
    {
        std::lock_guard<std::mutex> g(Fake::mu);
        if (Fake::call("scatter:" + Fake::name(Fake::dev, image, 'i') + ":" + Fake::name(Fake::pinned, ops, 'b') + ":" +
                       std::to_string(n) + ":s" + std::to_string(s)))
            return 2;
    }
    for (uint32_t i = 0; i < n; i++) {
        CHECK((int)ops[i].list >= last_list && ops[i].list == ops[0].list);
        last_list = (int)ops[i].list;
        image[ops[i].slot].v = ops[i].v;
    }
    return Fake::kOk;
}
static int update(Mirror& m, const std::vector<Op>& first, const std::vector<Op>& second, int s) {
    last_list = 0;
    return m.update(first, second, s, scatter);
}
// a read on s: which image it was given (logged as "launch:iK"), or -1
static int read(const Mirror& m, int s, const Slot** image = nullptr) {
    int got = -1;
    const int rc = m.read(s, [&](int k, const Slot* im) {
        got = k;
        if (image) *image = im;
        Fake::note("launch:i" + std::to_string(k));
        return Fake::kOk;
    });
    return rc == NEB_OK ? got : -1;
}
static std::vector<Op> ops_of(uint32_t n, uint32_t from, uint32_t list) {
    std::vector<Op> v(n);
    for (uint32_t i = 0; i < n; i++) v[i] = Op{from + i, list, ((uint64_t)list << 32) | (from + i)};
    return v;
}

// Updates take effect in call order: a stream wait only when the last update ran on another stream.
static void test_update_order() {
    Fake::reset();
    Mirror m;
    CHECK(m.init(64) == NEB_OK);
    CHECK((take() == Log{"alloc", "memset:i0", "halloc", "create:e0", "alloc", "memset:i1", "halloc", "create:e1", "halloc",
                         "create:e2", "dsync"}));
    CHECK(update(m, {}, {}, 1) == NEB_OK);  // nothing to send: no call at all
    CHECK(take().empty());
    CHECK(update(m, ops_of(1, 0, 1), {}, 1) == NEB_OK);  // the first update: nothing to wait for
    CHECK((take() == Log{"scatter:i0:b0:1:s1", "record:e0:s1", "record:e2:s1", "create:e3", "record:e3:s1"}));
    CHECK(update(m, ops_of(1, 1, 1), {}, 1) == NEB_OK);  // the stream of the previous update: ordered already
    CHECK((take() == Log{"scatter:i0:b1:1:s1", "record:e1:s1", "record:e2:s1", "record:e3:s1"}));
    CHECK(update(m, ops_of(1, 2, 1), ops_of(1, 3, 2), 2) == NEB_OK);  // another stream: one wait, before its first scatter
    CHECK((take() == Log{"wait:s2:e2", "sync:e0", "scatter:i0:b0:1:s2", "record:e0:s2", "sync:e1", "scatter:i0:b1:1:s2",
                         "record:e1:s2", "record:e2:s2", "create:e4", "record:e4:s2"}));
    CHECK(update(m, {}, ops_of(1, 4, 2), 2) == NEB_OK);
    CHECK(count(take(), "wait") == 0);
    // after a rebuild the new image has no update in flight: no wait on any stream
    std::vector<Slot> host(64);
    CHECK(m.rebuild(host.data(), 1) == NEB_OK);
    CHECK((take() == Log{"copy:i1:b2:s1", "ssync:s1"}));
    CHECK(update(m, ops_of(1, 5, 1), {}, 3) == NEB_OK);
    CHECK((take() == Log{"sync:e1", "scatter:i1:b1:1:s3", "record:e1:s3", "record:e2:s3", "create:e5", "record:e5:s3"}));
    CHECK(update(m, ops_of(1, 6, 1), {}, 1) == NEB_OK);
    CHECK(count(take(), "wait:s1:e2") == 1);
    m.drain();
}

// One update of n + n ops on a fresh mirror, then one more op: chunk sizes, buffer alternation, the
// host wait in front of a refill, `first` before `second`.
static void test_chunks(uint32_t n) {
    Fake::reset();
    Mirror m;
    CHECK(m.init(4 * kStage + 8) == NEB_OK);
    take();
    const std::vector<Op> first = ops_of(n, 0, 1), second = ops_of(n, 2 * kStage + 2, 2);
    CHECK(update(m, first, second, 7) == NEB_OK);
    CHECK(update(m, ops_of(1, 4 * kStage + 7, 1), {}, 7) == NEB_OK);
    const Log l = take();
    std::vector<uint32_t> want;  // the launches' sizes
    for (int list = 0; list < 2; list++)
        for (uint32_t at = 0; at < n; at += kStage) want.push_back(std::min(kStage, n - at));
    want.push_back(1);
    bool busy[2] = {false, false};
    size_t launch = 0;
    for (size_t i = 0; i < l.size(); i++) {
        if (starts(l[i], "sync")) {  // only in front of the launch that refills that event's buffer
            CHECK(i + 1 < l.size() && starts(l[i + 1], "scatter"));
            continue;
        }
        if (!starts(l[i], "scatter")) continue;
        const int b = (int)(launch & 1);  // the buffers alternate, from b0, across lists and calls
        CHECK(launch < want.size());
        CHECK(l[i] == "scatter:i0:b" + std::to_string(b) + ":" + std::to_string(want[launch]) + ":s7");
        const std::string wait = "sync:e" + std::to_string(b);  // e0 follows b0, e1 follows b1
        CHECK(busy[b] == (i > 0 && l[i - 1] == wait));
        CHECK(i + 1 < l.size() && l[i + 1] == "record:e" + std::to_string(b) + ":s7");
        busy[b] = true;
        launch++;
    }
    CHECK(launch == want.size());
    CHECK(count(l, "sync") == (want.size() > 2 ? want.size() - 2 : 0));
    CHECK(count(l, "wait") == 0 && count(l, "record:e2:s7") == 2 && count(l, "create") == 1);
    CHECK(l.back() == "record:e3:s7");
    const Slot* image = nullptr;
    CHECK(read(m, 7, &image) == 0);
    for (const Op& o : first) CHECK(image[o.slot].v == o.v);
    for (const Op& o : second) CHECK(image[o.slot].v == o.v);
    CHECK(image[n].v == 0 && image[4 * kStage + 7].v != 0);
    take();
    m.drain();
}

static void test_rebuild() {
    Fake::reset();
    Mirror m;
    std::vector<Slot> host(64);
    CHECK(m.init(64) == NEB_OK);
    CHECK(read(m, 1) == 0 && read(m, 2) == 0 && read(m, 1) == 0);  // image 0: e3 on s1, e4 on s2
    CHECK((take() == Log{"alloc", "memset:i0", "halloc", "create:e0", "alloc", "memset:i1", "halloc", "create:e1", "halloc",
                         "create:e2", "dsync", "launch:i0", "create:e3", "record:e3:s1", "launch:i0", "create:e4",
                         "record:e4:s2", "launch:i0", "record:e3:s1"}));
    host[5].v = 55;
    CHECK(m.rebuild(host.data(), 9) == NEB_OK);  // the spare image has no user yet
    CHECK((take() == Log{"copy:i1:b2:s9", "ssync:s9"}));
    CHECK(read(m, 1) == 1 && read(m, 3) == 1);  // image 1: e5 on s1, e6 on s3
    CHECK(update(m, ops_of(1, 6, 1), {}, 1) == NEB_OK);
    take();
    // image 0 again: the host waits for its two users and for none of image 1's; copy, whatever
    // travels with the image, sync, and only then the switch. A read meanwhile gets the old image.
    host[7].v = 77;
    int switched = -1;
    auto extra = [&](int spare, int s) {
        Fake::note("extra:i" + std::to_string(spare) + ":s" + std::to_string(s));
        CHECK(read(m, 2) == 1);
        return Fake::kOk;
    };
    auto on_switch = [&](int spare) {
        Fake::note("switch");
        switched = spare;
    };
    CHECK(m.rebuild(host.data(), 9, extra, on_switch) == NEB_OK);
    CHECK((take() == Log{"sync:e3", "sync:e4", "copy:i0:b2:s9", "extra:i0:s9", "launch:i1", "create:e7", "record:e7:s2",
                         "ssync:s9", "switch"}));
    CHECK(switched == 0);
    const Slot* image = nullptr;
    CHECK(read(m, 2, &image) == 0);
    CHECK(image[5].v == 55 && image[7].v == 77 && image[6].v == 0);  // the host copy, not the old image's update
    CHECK((take() == Log{"launch:i0", "record:e4:s2"}));
    // a failed call in the rebuild leaves the old image active
    Fake::fail_at = 2;
    CHECK(m.rebuild(host.data(), 9) == NEB_ERR_HIP);
    Fake::fail_at = 0;
    CHECK(read(m, 2) == 0);
    m.drain();
}

// init with its k-th device call failing, for every k: the error comes back, drain and the
// destructor are clean, and ASan's leak check sees what the fake handed out.
static void test_init_failures() {
    Fake::reset();
    size_t calls;
    {
        Mirror m;
        CHECK(m.init(64) == NEB_OK);
        calls = take().size();
        m.drain();
    }
    CHECK(calls == 11);
    for (size_t k = 1; k <= calls; k++) {
        Fake::reset();
        Fake::fail_at = (int)k;
        {
            Mirror m;
            CHECK(m.init(64) == NEB_ERR_HIP);
            CHECK(take().size() == k && Fake::fail_at == 0);
            m.drain();  // waits for the events that exist, recorded or not; nothing else
            const Log d = take();
            CHECK(count(d, "sync:") == d.size() && d.size() <= 3);
        }
        CHECK(Fake::events.empty() && Fake::dev.empty() && Fake::pinned.empty());
    }
}

// drain waits for every event that was ever recorded (the fake checks at every destroy and free
// that nothing is pending).
static void test_drain() {
    Fake::reset();
    Mirror m;
    std::vector<Slot> host(2 * kStage + 64);
    CHECK(m.init(host.size()) == NEB_OK);
    for (int s = 1; s <= 3; s++) CHECK(read(m, s) == 0);
    CHECK(update(m, ops_of(kStage + 1, 0, 1), ops_of(3, kStage + 10, 2), 4) == NEB_OK);
    CHECK(m.rebuild(host.data(), 5) == NEB_OK);
    for (int s = 2; s <= 6; s++) CHECK(read(m, s) == 1);
    CHECK(update(m, ops_of(2, 0, 1), {}, 6) == NEB_OK);
    std::set<std::string> recorded;
    for (const std::string& c : take())
        if (starts(c, "record:")) recorded.insert(c.substr(7, c.find(':', 7) - 7));
    CHECK(recorded.size() == 3 + 4 + 5);  // staging and update events, image 0's users, image 1's
    m.drain();
    const Log l = take();
    for (const std::string& e : recorded) CHECK(std::count(l.begin(), l.end(), "sync:" + e) == 1);
    CHECK(l.size() == recorded.size());
    for (FakeEvent* ev : Fake::events) CHECK(!ev->pending);
}

// Random updates and rebuilds from a seeded generator: after each, the active image is the host copy.
static void test_random() {
    Fake::reset();
    Fake::logging = false;
    std::mt19937 rng(20261);
    constexpr uint32_t kSlots = 3 * kStage;
    Mirror m;
    std::vector<Slot> host(kSlots);
    CHECK(m.init(kSlots) == NEB_OK);
    std::vector<uint32_t> perm(kSlots);
    for (uint32_t i = 0; i < kSlots; i++) perm[i] = i;
    for (int round = 0; round < 3000; round++) {
        const int s = 1 + (int)(rng() % 4);
        if (rng() % 16 == 0) {
            for (uint32_t i = 0; i < 64; i++) host[rng() % kSlots].v = rng();
            CHECK(m.rebuild(host.data(), s) == NEB_OK);
        } else {
            // mostly small; now and then larger than one or two staging buffers. Distinct slots
            // within a list; a slot of `first` may come again in `second`, whose value then stands
            const uint32_t big = rng() % 64 == 0 ? kStage + rng() % (kStage + 2) : 0;
            std::vector<Op> first(rng() % 4 + big), second(rng() % 4);
            for (size_t i = 0; i < first.size(); i++) {
                std::swap(perm[i], perm[i + rng() % (kSlots - i)]);
                first[i] = Op{perm[i], 1, rng()};
            }
            for (size_t i = 0; i < second.size(); i++) {
                const size_t at = first.size() + i;
                std::swap(perm[at], perm[at + rng() % (kSlots - at)]);
                second[i] = Op{!first.empty() && rng() % 2 ? first[i % first.size()].slot : perm[at], 2, rng()};
                for (size_t j = 0; j < i; j++)
                    if (second[j].slot == second[i].slot) second[i].slot = perm[at];
            }
            for (const Op& o : first) host[o.slot].v = o.v;
            for (const Op& o : second) host[o.slot].v = o.v;
            CHECK(update(m, first, second, s) == NEB_OK);
        }
        const Slot* image = nullptr;
        CHECK(read(m, 1 + (int)(rng() % 4), &image) >= 0);
        CHECK(image && std::memcmp(image, host.data(), kSlots * sizeof(Slot)) == 0);
    }
    m.drain();
    Fake::logging = true;
}

// Two threads read on their own streams while one updates and rebuilds (the owner's writers are
// serialised; the reads take the mirror's lock alone).
static void test_threads() {
    Fake::reset();
    Fake::logging = false;
    Mirror m;
    std::vector<Slot> host(256);
    CHECK(m.init(host.size()) == NEB_OK);
    bool stop = false;
    std::mutex stop_mu;
    auto stopped = [&] {
        std::lock_guard<std::mutex> g(stop_mu);
        return stop;
    };
    auto reader = [&](int s) {
        size_t seen[2] = {0, 0};
        while (!stopped()) {
            const int k = read(m, s);
            CHECK(k == 0 || k == 1);
            if (k >= 0) seen[k]++;
        }
        CHECK(seen[0] + seen[1] > 0);
    };
    std::thread r1(reader, 1), r2(reader, 2);
    std::mt19937 rng(5);
    for (int round = 0; round < 2000; round++) {
        const int s = 3 + (int)(rng() % 2);
        if (round % 50 == 49) CHECK(m.rebuild(host.data(), s) == NEB_OK);
        else CHECK(update(m, ops_of(1 + rng() % 3, rng() % 200, 1), ops_of(rng() % 2, 210 + rng() % 40, 2), s) == NEB_OK);
    }
    {
        std::lock_guard<std::mutex> g(stop_mu);
        stop = true;
    }
    r1.join();
    r2.join();
    m.drain();
    Fake::logging = true;
}

int main() {
    test_update_order();
    for (uint32_t n : {1u, kStage, kStage + 1u, 2u * kStage + 1u}) test_chunks(n);
    test_rebuild();
    test_init_failures();
    test_drain();
    test_random();
    test_threads();
    CHECK(Fake::events.empty() && Fake::dev.empty() && Fake::pinned.empty());  // every mirror tore itself down
    if (fails) {
        std::fprintf(stderr, "mirror_test: %d failures\n", fails);
        return 1;
    }
    std::printf("mirror_test: ok\n");
    return 0;
}
