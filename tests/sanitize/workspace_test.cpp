// workspace_test.cpp — sanitizer test (ASan + UBSan, and TSan) of the device workspace protocol
// (nebula_amd/csrc/workspace.hpp) over a fake device: it logs every call, gives a stream a handle
// and an id, keeps each recorded event "pending" until the host has waited for it, and aborts when
// memory is freed while an event recorded after that memory's last use is still pending. The test
// pins which ordering calls reserve / begin / end / destroy make and in which order; ASan's leak
// check covers the fake's allocations and events. TEST INFRASTRUCTURE; `make -C tests/sanitize`.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../nebula_amd/csrc/workspace.hpp"

static int fails = 0;
#define CHECK(x)                                                                              \
    do {                                                                                      \
        if (!(x)) {                                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x);        \
            fails++;                                                                          \
        }                                                                                     \
    } while (0)

struct FakeEvent {
    uint64_t seq = 0;      // when it was last recorded
    bool pending = false;  // recorded, and the host has not waited for it since
};

struct Fake {
    using Stream = const void*;
    using Event = FakeEvent*;
    using Error = int;
    static constexpr int kOk = 0;

    // the fake device's state (one workspace protocol at a time; the threaded part holds a mutex)
    static inline std::vector<std::string> log;
    static inline std::map<const void*, unsigned long long> ids;  // stream handle -> its id
    static inline bool have_ids = true;                           // false: the runtime has no id lookup
    static inline bool fail_alloc = false;
    static inline uint64_t seq = 0;
    static inline std::set<FakeEvent*> events;
    static inline std::map<uint8_t*, uint64_t> last_use;  // live allocations -> their last use

    static void use(uint8_t* p) {  // a kernel that works in p was enqueued
        CHECK(last_use.count(p) == 1);
        last_use[p] = ++seq;
    }

    static int event_create(Event* ev) {
        log.push_back("create");
        *ev = new FakeEvent;
        events.insert(*ev);
        return kOk;
    }
    static int event_sync(Event ev) {
        log.push_back("sync");
        ev->pending = false;
        return kOk;
    }
    static int event_record(Event ev, Stream) {
        log.push_back("record");
        ev->seq = ++seq;
        ev->pending = true;
        return kOk;
    }
    static void event_destroy(Event ev) {
        log.push_back("destroy");
        events.erase(ev);
        delete ev;
    }
    static int stream_wait(Stream, Event) {
        log.push_back("wait");
        return kOk;
    }
    static unsigned long long stream_id(Stream s) { return have_ids ? ids[s] : 0ull; }
    static int mem_alloc(uint8_t** p, size_t bytes) {
        log.push_back("alloc");
        if (fail_alloc) return 2;
        *p = static_cast<uint8_t*>(std::malloc(bytes));
        last_use[*p] = 0;
        return kOk;
    }
    static void mem_free(uint8_t* p) {
        log.push_back("free");
        for (FakeEvent* ev : events)
            if (ev->pending && ev->seq > last_use.at(p)) {
                std::fprintf(stderr, "workspace_test: memory freed while a batch recorded after its last use is pending\n");
                std::abort();
            }
        last_use.erase(p);
        std::free(p);
    }
};

using Ws = neb::DevWorkspace<Fake>;
using Log = std::vector<std::string>;

// the calls since the last take()
static Log take() {
    Log l;
    l.swap(Fake::log);
    return l;
}

// one batch on stream s in a workspace of `bytes`: the calls it made
static Log batch(Ws& w, size_t bytes, Fake::Stream s, bool* grew = nullptr) {
    CHECK(w.reserve(bytes, grew) == Fake::kOk);
    CHECK(w.begin(s) == Fake::kOk);
    Fake::use(w.mem());
    CHECK(w.end(s) == Fake::kOk);
    return take();
}

static void test_stream_rule() {
    int a = 0, b = 0;  // two streams: their addresses are the handles
    Fake::ids = {{&a, 11}, {&b, 12}};
    Fake::have_ids = true;
    Ws w;
    bool grew = false;
    // the first begin creates the event and waits for nothing
    CHECK((batch(w, 1000, &a, &grew) == Log{"alloc", "create", "record"}));
    CHECK(grew && w.bytes() == 1000 && w.mem());
    // the stream of the last end: ordered already, no wait; capacity suffices: no call
    CHECK((batch(w, 1000, &a, &grew) == Log{"record"}));
    CHECK(!grew);
    CHECK((batch(w, 10, &a) == Log{"record"}));
    // another stream: exactly one wait
    CHECK((batch(w, 1000, &b) == Log{"wait", "record"}));
    CHECK((batch(w, 1000, &b) == Log{"record"}));
    // the same handle with a new id (b destroyed, a new stream at its address): a wait
    Fake::ids[&b] = 13;
    CHECK((batch(w, 1000, &b) == Log{"wait", "record"}));
    CHECK((batch(w, 1000, &b) == Log{"record"}));
    // no id lookup in the runtime: the handle alone decides
    Fake::have_ids = false;
    CHECK((batch(w, 1000, &a) == Log{"wait", "record"}));
    Fake::ids[&a] = 99;
    CHECK((batch(w, 1000, &a) == Log{"record"}));
    CHECK((batch(w, 1000, &b) == Log{"wait", "record"}));
    Fake::have_ids = true;
    // a batch that binds the event to its own last kernel: end_bound remembers the stream only
    CHECK(w.reserve(1000) == Fake::kOk && w.begin(&a) == Fake::kOk);
    CHECK(w.event() != nullptr);
    w.end_bound(&a);
    CHECK((take() == Log{"wait"}));
    CHECK(w.begin(&a) == Fake::kOk);
    CHECK(take().empty());
    // teardown: waits for the last batch, destroys the event, frees
    w.destroy();
    CHECK((take() == Log{"sync", "destroy", "free"}));
    CHECK(!w.mem() && w.bytes() == 0 && !w.event());
    w.destroy();  // (and again by the destructor: nothing left to do)
    CHECK(take().empty());
}

static void test_growth() {
    int a = 0, b = 0;
    Fake::ids = {{&a, 1}, {&b, 2}};
    Ws w;
    bool grew = true;
    CHECK(w.reserve(0, &grew) == Fake::kOk);  // nothing yet: even 0 bytes allocates
    CHECK(grew);
    take();
    batch(w, 64, &a);
    // growing while the last batch is pending: the host waits for it, then frees, then allocates
    // (the fake aborts in mem_free if the wait is missing)
    CHECK(w.reserve(4096, &grew) == Fake::kOk);
    CHECK((take() == Log{"sync", "free", "alloc"}));
    CHECK(grew && w.bytes() == 4096 && w.mem());
    // the grown workspace on another stream: ordered behind the event like any batch
    CHECK((batch(w, 4096, &b) == Log{"wait", "record"}));
    // a failed allocation: empty, capacity 0, and the next reserve allocates again
    Fake::fail_alloc = true;
    CHECK(w.reserve(1 << 20, &grew) != Fake::kOk);
    CHECK((take() == Log{"sync", "free", "alloc"}));
    CHECK(!grew && !w.mem() && w.bytes() == 0);
    Fake::fail_alloc = false;
    CHECK(w.reserve(64, &grew) == Fake::kOk);
    CHECK((take() == Log{"sync", "alloc"}));
    CHECK(grew && w.bytes() == 64);
    batch(w, 64, &a);
    // the destructor tears down what is left
}

// two buffers ordered by one event (the transmit batch's workspace and its host staging)
static void test_two_buffers() {
    int a = 0;
    Fake::ids = {{&a, 1}};
    {
        neb::DevWorkspace<Fake, 2> w;
        bool grew = false;
        CHECK(w.reserve(100, &grew, 0) == Fake::kOk && grew);
        CHECK(w.reserve(200, &grew, 1) == Fake::kOk && grew);
        CHECK(w.mem(0) != w.mem(1) && w.bytes(0) == 100 && w.bytes(1) == 200);
        CHECK(w.begin(&a) == Fake::kOk);
        Fake::use(w.mem(0));
        Fake::use(w.mem(1));
        CHECK(w.end(&a) == Fake::kOk);
        take();
        CHECK(w.reserve(100, &grew, 0) == Fake::kOk && !grew);
        CHECK(take().empty());
        CHECK(w.reserve(300, &grew, 1) == Fake::kOk && grew);  // the pending batch uses it too
        CHECK((take() == Log{"sync", "free", "alloc"}));
        CHECK(w.bytes(0) == 100 && w.bytes(1) == 300);
    }
    CHECK((take() == Log{"sync", "destroy", "free", "free"}));
}

// batches from two threads, each on its own stream, under the owner's mutex as the engine holds it
static void test_threads() {
    int s[2] = {0, 0};
    Fake::ids = {{&s[0], 1}, {&s[1], 2}};
    Ws w;
    std::mutex mu;
    size_t waits = 0;
    auto run = [&](int t) {
        for (int i = 0; i < 200; i++) {
            std::lock_guard<std::mutex> g(mu);
            for (const std::string& c : batch(w, 64 + (size_t)(i / 50) * 1000 * (size_t)(t + 1), &s[t])) waits += c == "wait";
        }
    };
    std::thread t0(run, 0), t1(run, 1);
    t0.join();
    t1.join();
    CHECK(waits >= 1 && waits < 400);
    take();
}

int main() {
    test_stream_rule();
    test_growth();
    test_two_buffers();
    test_threads();
    CHECK(Fake::events.empty() && Fake::last_use.empty());  // every workspace tore itself down
    if (fails) {
        std::fprintf(stderr, "workspace_test: %d failures\n", fails);
        return 1;
    }
    std::printf("workspace_test: ok\n");
    return 0;
}
