// comb_test.cpp — sanitizer test (ASan + UBSan, and TSan) of the per-packet combiner's state machine
// (nebula_amd/csrc/comb_core.hpp) on a fake device. The test holds and releases the completion of
// every launch, alone or combined, so which calls gather into which batch is scripted, not left to
// timing; the fake computes every result with the plain-C oracle (oracle/aead_oracle.c, test
// infrastructure), can fail a combined launch, and can leave a launch's statuses unpublished until
// the leader falls back to waiting for the launch. Every caller's result bytes and status must
// equal the oracle run directly on its request. Every wait is bounded: a scenario that takes more
// than 60 s (a lost wake-up) ends the program with a failure. TEST INFRASTRUCTURE;
// `make -C tests/sanitize`.
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <functional>
#include <random>
#include <thread>

#include "../../nebula_amd/csrc/comb_core.hpp"

extern "C" void ora_batch(int alg, int open, const uint8_t* keys, const neb_desc* d, size_t n, uint8_t* arena,
                          int32_t* status);

static std::atomic<int> fails{0};
#define CHECK(x)                                                                              \
    do {                                                                                      \
        if (!(x)) {                                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x);        \
            fails++;                                                                          \
        }                                                                                     \
    } while (0)

using neb::kCombMax;
using neb::kCombSlot;
using Clock = std::chrono::steady_clock;
constexpr auto kLimit = std::chrono::seconds(60);
constexpr uint32_t kKeys = 8;
static uint8_t g_keys[32 * kKeys];

// (a deadline on the system clock: the sanitizer's runtime follows that wait of a condition
// variable, not the steady clock's)
static std::chrono::system_clock::time_point wall_limit() { return std::chrono::system_clock::now() + kLimit; }

[[noreturn]] static void die(const char* what) {
    std::fprintf(stderr, "comb_test: FAILED: %s\n", what);
    std::fflush(nullptr);
    _exit(1);
}

// Poll until pred() holds, 60 s at the most.
template <class P>
static void wait_for(P pred, const char* what) {
    const auto end = Clock::now() + kLimit;
    while (!pred()) {
        if (Clock::now() > end) die(what);
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

// Ends the program when its scenario has not finished within 60 s.
struct Watchdog {
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    std::thread th;
    explicit Watchdog(const char* name)
        : th([this, name] {
              std::unique_lock<std::mutex> lk(mu);
              if (!cv.wait_until(lk, wall_limit(), [&] { return done; })) die(name);
          }) {}
    ~Watchdog() {
        {
            std::lock_guard<std::mutex> g(mu);
            done = true;
        }
        cv.notify_all();
        th.join();
    }
};

// One request against the oracle: the status, and the bytes of the arena [aad pad 16 | payload (+ tag)]
static int32_t oracle_run(int alg, int open, uint32_t key, uint64_t ctr, size_t ad_len, size_t pay_len,
                          std::vector<uint8_t>& arena) {
    if (key >= kKeys) return NEB_STATUS_BAD_KEY;
    neb_desc d{};
    d.src_off = d.dst_off = neb::comb_pay(ad_len);
    d.counter = ctr;
    d.len = (uint32_t)pay_len;
    d.aad_len = (uint32_t)ad_len;
    d.key_id = key;
    int32_t st = -1;
    ora_batch(alg, open, g_keys, &d, 1, arena.data(), &st);
    return st;
}

// ---- the fake device ---------------------------------------------------------------------------

struct Job {
    bool combined = false;
    int open = 0;
    uint32_t n = 1, turn = 0;
    std::vector<neb_desc> descs;  // a combined launch's descriptors as the launch took them
    int32_t* status = nullptr;
    uint8_t* slots = nullptr;
    bool publish = true;                 // false: the statuses appear only when the leader waits for the launch
    std::vector<int32_t> held_status;
    bool released = false, computed = false, published = false;  // (FakeDev::mu)
};

struct FakeDev {
    struct Buf {
        std::unique_ptr<uint8_t[]> p;
        operator uint8_t*() const { return p.get(); }
    };
    using Token = std::shared_ptr<Job>;
    struct Guard {
        explicit Guard(FakeDev& d) { d.guards++; }
    };
    std::mutex mu;
    std::condition_variable cv;
    std::vector<Token> jobs;  // every launch, alone or combined, in launch order
    int fail_combined = 0;    // the next so many combined launches fail
    int unpublish_combined = 0;  // the next so many combined launches leave their statuses unpublished
    uint32_t unpublish_every = 0;  // and every so-manieth one after them
    std::atomic<uint64_t> guards{0}, reserves{0}, solo_calls{0}, counted{0}, syncs{0}, failed_launches{0};

    bool reserve(Buf& h, size_t bytes) {
        h.p.reset(new uint8_t[bytes]);
        std::memset(h.p.get(), 0xEE, bytes);
        reserves++;
        return true;
    }
    void wait_locked(std::unique_lock<std::mutex>& lk, const std::function<bool()>& pred, const char* what) {
        if (!cv.wait_until(lk, wall_limit(), pred)) die(what);
    }
    int solo(const neb::CombReq& q, int32_t* st) {
        Token j = std::make_shared<Job>();
        j->open = q.open;
        {
            std::unique_lock<std::mutex> lk(mu);
            jobs.push_back(j);
            cv.notify_all();
            wait_locked(lk, [&] { return j->released; }, "a call alone was never released");
        }
        const size_t pay = neb::comb_pay(q.ad_len);
        std::vector<uint8_t> arena(pay + std::max(q.in_len, q.pay_len + 16) + 16);
        if (q.ad_len) std::memcpy(arena.data(), q.ad, q.ad_len);
        if (q.in_len) std::memcpy(arena.data() + pay, q.in, q.in_len);
        const int32_t s = oracle_run(q.alg, q.open, q.key_id, q.n, q.ad_len, q.pay_len, arena);
        *st = s;
        neb::copy_result(q.open, s, q.dst, arena.data() + pay, q.pay_len);
        solo_calls++;
        std::lock_guard<std::mutex> g(mu);
        j->computed = true;
        cv.notify_all();
        return NEB_OK;
    }
    bool launch(int open, const neb_desc* desc, int32_t* status, uint8_t* slots, uint32_t n, uint32_t turn, Token& tok) {
        std::lock_guard<std::mutex> g(mu);
        if (fail_combined > 0) {
            fail_combined--;
            failed_launches++;
            return false;
        }
        Token j = std::make_shared<Job>();
        j->combined = true;
        j->open = open;
        j->n = n;
        j->turn = turn;
        j->descs.assign(desc, desc + n);
        j->status = status;
        j->slots = slots;
        if (unpublish_combined > 0) {
            unpublish_combined--;
            j->publish = false;
        } else if (unpublish_every && turn % unpublish_every == 0) {
            j->publish = false;
        }
        jobs.push_back(j);
        tok = j;
        cv.notify_all();
        return true;
    }
    bool poll(Token& j, const int32_t* p) {
        std::unique_lock<std::mutex> lk(mu);
        wait_locked(lk, [&] { return j->computed; }, "a combined launch was never released");
        return j->published && __atomic_load_n(p, __ATOMIC_ACQUIRE) != -1;
    }
    bool sync(Token& j) {
        std::unique_lock<std::mutex> lk(mu);
        wait_locked(lk, [&] { return j->computed; }, "a combined launch was never released");
        syncs++;
        if (!j->published) {
            for (uint32_t i = 0; i < j->n; i++) __atomic_store_n(j->status + i, j->held_status[i], __ATOMIC_RELEASE);
            j->published = true;
        }
        return true;
    }
    void count(uint32_t n) { counted += n; }

    // -- the test's side: the launch completes --
    void release(const Token& j) {
        if (j->combined) {  // the kernel: every request in its slot, then its status
            std::vector<int32_t> st(j->n);
            for (uint32_t i = 0; i < j->n; i++) {
                st[i] = NEB_STATUS_BAD_KEY;
                if (j->descs[i].key_id < kKeys) ora_batch(NEB_ALG_AESGCM, j->open, g_keys, &j->descs[i], 1, j->slots, &st[i]);
            }
            if (j->publish)
                for (uint32_t i = 0; i < j->n; i++) __atomic_store_n(j->status + i, st[i], __ATOMIC_RELEASE);
            std::lock_guard<std::mutex> g(mu);
            j->held_status = st;
            j->released = j->computed = true;
            j->published = j->publish;
        } else {
            std::lock_guard<std::mutex> g(mu);
            j->released = true;
        }
        cv.notify_all();
    }
    size_t njobs() {
        std::lock_guard<std::mutex> g(mu);
        return jobs.size();
    }
    Token job(size_t k) {
        std::lock_guard<std::mutex> g(mu);
        return jobs.at(k);
    }
    Token pick_unreleased(std::mt19937_64& rng) {  // any launch still held, or null
        std::lock_guard<std::mutex> g(mu);
        std::vector<Token> held;
        for (auto& j : jobs)
            if (!j->released) held.push_back(j);
        return held.empty() ? nullptr : held[rng() % held.size()];
    }
    void release_all() {
        for (size_t k = 0; k < njobs(); k++) {
            Token j = job(k);
            bool rel;
            {
                std::lock_guard<std::mutex> g(mu);
                rel = j->released;
            }
            if (!rel) release(j);
        }
    }
};

using Core = neb::CombCore<FakeDev>;

// ---- one caller's request and what the oracle says it must get ---------------------------------

constexpr size_t kGuard = 16;
struct Call {
    neb::CombReq q;
    std::vector<uint8_t> ad, in, out, exp_out;
    int32_t st = -77, exp_st = -1;
    int rc = -99;
    std::thread th;
};

enum { kClean = 0, kForged = 1 };
static void make_call(Call& c, std::mt19937_64& rng, int alg, int open, size_t ad_len, size_t pay_len, uint32_t key,
                      uint64_t ctr, int forged = kClean) {
    const size_t pay = neb::comb_pay(ad_len);
    std::vector<uint8_t> arena(pay + pay_len + 16);
    for (auto& b : arena) b = (uint8_t)rng();
    c.ad.assign(arena.begin(), arena.begin() + ad_len);
    if (open) {  // seal first (an uninstalled key opens whatever bytes there are)
        oracle_run(alg, 0, key, ctr, ad_len, pay_len, arena);
        if (forged) arena[pay + rng() % (pay_len + 16)] ^= 0x10;
        c.in.assign(arena.begin() + pay, arena.begin() + pay + pay_len + 16);
    } else {
        c.in.assign(arena.begin() + pay, arena.begin() + pay + pay_len);
    }
    const size_t out_len = open ? pay_len : pay_len + 16;
    c.exp_st = oracle_run(alg, open, key, ctr, ad_len, pay_len, arena);
    c.out.assign(out_len + kGuard, 0xAA);
    c.exp_out = c.out;
    if (c.exp_st == NEB_STATUS_OK) std::copy(arena.begin() + pay, arena.begin() + pay + out_len, c.exp_out.begin());
    else if (open && c.exp_st == NEB_STATUS_AUTH_FAILED) std::fill(c.exp_out.begin(), c.exp_out.begin() + out_len, 0);
    c.q.alg = alg;
    c.q.open = open;
    c.q.key_id = key;
    c.q.n = ctr;
    c.q.ad = c.ad.data();
    c.q.ad_len = ad_len;
    c.q.in = c.in.data();
    c.q.in_len = c.in.size();
    c.q.pay_len = pay_len;
    c.q.dst = c.out.data();
}
static bool call_ok(const Call& c) { return c.rc == NEB_OK && c.st == c.exp_st && c.out == c.exp_out; }
// a failed launch: NEB_ERR_HIP, no output and no status written
static bool call_untouched(const Call& c) {
    return c.rc == NEB_ERR_HIP && c.st == -77 && std::all_of(c.out.begin(), c.out.end(), [](uint8_t b) { return b == 0xAA; });
}

// The calls of a scripted scenario, each on a thread of its own.
struct Script {
    Core& core;
    std::mt19937_64 rng;
    std::deque<Call> calls;
    uint64_t ctr = 1000;
    Script(Core& c, uint64_t seed) : core(c), rng(seed) {}
    size_t start(int open, size_t ad_len, size_t pay_len, uint32_t key = 1, int alg = NEB_ALG_AESGCM, int forged = kClean) {
        calls.emplace_back();
        Call& c = calls.back();
        make_call(c, rng, alg, open, ad_len, pay_len, key, ctr++, forged);
        c.th = std::thread([this, &c] { c.rc = core.call(c.q, &c.st); });
        return calls.size() - 1;
    }
    // a call that must go alone and be held there: started, and seen as the device's launch number `at`
    size_t start_alone(size_t at, int open = 0, size_t ad_len = 16, size_t pay_len = 100, int alg = NEB_ALG_AESGCM) {
        const size_t k = start(open, ad_len, pay_len, 1, alg);
        wait_for([&] { return core.dev.njobs() == at + 1; }, "a call did not launch alone");
        CHECK(!core.dev.job(at)->combined);
        return k;
    }
    // a call that must join the gathering batch of its direction as request number `as`
    size_t start_joining(uint32_t as, int open, size_t ad_len, size_t pay_len, uint32_t key = 1, int forged = kClean) {
        const uint32_t before = core.state().gathering;
        const size_t k = start(open, ad_len, pay_len, key, NEB_ALG_AESGCM, forged);
        wait_for([&] { return core.state().gathering == before + 1; }, "a call did not join a batch");
        const uint32_t now = core.state().open_n[open ? 1 : 0];
        CHECK(now == (as + 1) % kCombMax);  // (a full batch is no longer the open one)
        return k;
    }
    void join(size_t k) {
        if (calls[k].th.joinable()) calls[k].th.join();
    }
    void finish_ok(size_t k) {
        join(k);
        CHECK(call_ok(calls[k]));
    }
    void finish_all_ok() {
        for (size_t k = 0; k < calls.size(); k++) finish_ok(k);
    }
    // a combined launch carries exactly calls[first...] in join order, request r in slot r
    void check_carries(const FakeDev::Token& j, const std::vector<size_t>& which, int open) {
        CHECK(j->combined && j->open == open && j->n == which.size());
        for (size_t r = 0; r < which.size() && r < j->n; r++) {
            const neb::CombReq& q = calls[which[r]].q;
            const neb_desc& d = j->descs[r];
            CHECK(d.counter == q.n && d.len == q.pay_len && d.aad_len == q.ad_len && d.key_id == q.key_id);
            CHECK(d.aad_off == r * (uint64_t)kCombSlot && d.src_off == d.aad_off + neb::comb_pay(q.ad_len) && d.dst_off == d.src_off);
        }
    }
};

static void check_idle(Core& core) {
    const Core::State s = core.state();
    CHECK(s.inflight == 0 && s.solo == 0 && s.free_batches == s.batches && s.gathering == 0);
    CHECK(s.open_n[0] == 0 && s.open_n[1] == 0);
}
static std::vector<uint64_t> counters(Core& core) {
    uint64_t c[2];
    core.counters(c);
    return {c[0], c[1]};
}
using U64s = std::vector<uint64_t>;

// ---- 1: gathering under held launches ------------------------------------------------------------
static void gathering() {
    Watchdog wd("gathering under held launches");
    Core core(4, 4);
    FakeDev& dev = core.dev;
    Script s(core, 1);
    for (size_t i = 0; i < 4; i++) s.start_alone(i);  // up to the limit, calls go alone
    Core::State st = core.state();
    CHECK(st.inflight == 4 && st.solo == 4 && st.batches == 0);
    const size_t lead = s.start_joining(0, 0, 13, 0);   // the next one opens a batch and leads it
    const size_t j1 = s.start_joining(1, 0, 0, 2032);   // later ones join
    const size_t j2 = s.start_joining(2, 0, 1348, 0, 9);  // (an uninstalled key rides along)
    // nothing launches while every slot is held
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    CHECK(dev.njobs() == 4 && counters(core) == (U64s{0, 0}));
    st = core.state();
    CHECK(st.inflight == 4 && st.batches == 1 && st.free_batches == 0 && st.gathering == 3);
    // one launch completes: exactly one combined launch, the joined requests in join order
    dev.release(dev.job(0));
    s.finish_ok(0);
    wait_for([&] { return dev.njobs() == 5; }, "the leader did not launch");
    const FakeDev::Token b1 = dev.job(4);
    s.check_carries(b1, {lead, j1, j2}, 0);
    wait_for([&] { return counters(core) == (U64s{1, 3}); }, "the launch was not counted");  // (counted after the launch call)
    CHECK(dev.counted == 3);
    st = core.state();
    CHECK(st.inflight == 4 && st.solo == 3 && st.gathering == 0 && st.open_n[0] == 0 && st.free_batches == 0);
    // a call that arrives now cannot join the launched batch: it opens the next one (a second buffer)
    const size_t late = s.start_joining(0, 0, 16, 64);
    CHECK(core.state().batches == 2);
    dev.release(b1);
    for (size_t k : {lead, j1, j2}) s.finish_ok(k);  // each owner its own result
    CHECK(s.calls[j2].st == NEB_STATUS_BAD_KEY);
    // the batch is back on the free list once its last owner has copied out; `late` launches now
    wait_for([&] { return dev.njobs() == 6; }, "the second leader did not launch");
    CHECK(core.state().free_batches == 1);
    s.check_carries(dev.job(5), {late}, 0);
    // the next batch reuses the first one's buffer
    const size_t again = s.start_joining(0, 0, 17, 5);
    CHECK(core.state().batches == 2 && core.state().free_batches == 0);
    dev.release(dev.job(5));
    s.finish_ok(late);
    wait_for([&] { return dev.njobs() == 7; }, "the third leader did not launch");
    CHECK(dev.job(6)->slots == b1->slots && dev.reserves == 2);
    s.check_carries(dev.job(6), {again}, 0);
    dev.release_all();
    s.finish_all_ok();
    check_idle(core);
    CHECK(counters(core) == (U64s{3, 5}) && dev.solo_calls == 4 && dev.syncs == 0);
}

// ---- 2: a full batch -----------------------------------------------------------------------------
static void full_batch() {
    Watchdog wd("a full batch");
    Core core(1, 4);
    FakeDev& dev = core.dev;
    Script s(core, 2);
    s.start_alone(0);
    std::vector<size_t> first, second;
    for (uint32_t r = 0; r < kCombMax; r++) first.push_back(s.start_joining(r, 0, r % 20, 3 * r));
    CHECK(core.state().open_n[0] == 0 && core.state().gathering == kCombMax);  // closed by its kCombMax-th request
    second.push_back(s.start_joining(0, 0, 16, 1));  // the next call opens a second batch with its own leader
    second.push_back(s.start_joining(1, 0, 16, 2));
    CHECK(core.state().batches == 2 && dev.njobs() == 1);
    dev.release(dev.job(0));
    s.finish_ok(0);
    // both launch as slots free up, one at a time (the limit is 1), in either order
    wait_for([&] { return dev.njobs() == 2; }, "no leader launched");
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    CHECK(dev.njobs() == 2 && core.state().inflight == 1);
    const bool full_first = dev.job(1)->n == kCombMax;
    s.check_carries(dev.job(1), full_first ? first : second, 0);
    dev.release(dev.job(1));
    wait_for([&] { return dev.njobs() == 3; }, "the other leader did not launch");
    s.check_carries(dev.job(2), full_first ? second : first, 0);
    dev.release(dev.job(2));
    s.finish_all_ok();
    check_idle(core);
    CHECK(counters(core) == (U64s{2, kCombMax + 2}));
}

// ---- 3: directions -------------------------------------------------------------------------------
static void directions() {
    Watchdog wd("directions");
    Core core(1, 4);
    FakeDev& dev = core.dev;
    Script s(core, 3);
    s.start_alone(0, 1);
    const size_t s0 = s.start_joining(0, 0, 16, 100), o0 = s.start_joining(0, 1, 16, 100);
    const size_t s1 = s.start_joining(1, 0, 1, 33), o1 = s.start_joining(1, 1, 13, 0, 1, kForged);
    const size_t o2 = s.start_joining(2, 1, 0, 1300);
    CHECK(core.state().batches == 2 && core.state().open_n[0] == 2 && core.state().open_n[1] == 3);
    dev.release(dev.job(0));
    wait_for([&] { return dev.njobs() == 2; }, "no leader launched");
    const int first_open = dev.job(1)->open;
    dev.release(dev.job(1));
    wait_for([&] { return dev.njobs() == 3; }, "the other leader did not launch");
    CHECK(dev.job(2)->open == !first_open);
    s.check_carries(dev.job(first_open ? 2 : 1), {s0, s1}, 0);
    s.check_carries(dev.job(first_open ? 1 : 2), {o0, o1, o2}, 1);
    dev.release(dev.job(2));
    s.finish_all_ok();
    CHECK(s.calls[o1].st == NEB_STATUS_AUTH_FAILED);
    check_idle(core);
}

// ---- 4: ineligible calls -------------------------------------------------------------------------
static void ineligible() {
    Watchdog wd("ineligible calls");
    Core core(1, 4);
    FakeDev& dev = core.dev;
    Script s(core, 4);
    s.start_alone(0);
    const size_t a = s.start_joining(0, 0, 16, 10);
    // the other algorithm, one byte past the slot's input limit, and a result past the slot: alone,
    // outside the combiner's accounting, while the batch gathers
    const size_t cha = s.start_alone(1, 0, 16, 100, NEB_ALG_CHACHAPOLY);
    const size_t big = s.start_alone(2, 0, 16, 2033);
    const size_t big_open = s.start_alone(3, 1, 1348, 2048 - 1360 - 16 + 1);
    Core::State st = core.state();
    CHECK(st.inflight == 1 && st.solo == 1 && st.open_n[0] == 1 && st.gathering == 1);
    for (size_t k = 1; k <= 3; k++) dev.release(dev.job(k));
    for (size_t k : {cha, big, big_open}) s.finish_ok(k);
    const size_t b = s.start_joining(1, 0, 16, 2032);  // at the limit: joins
    st = core.state();
    CHECK(st.inflight == 1 && st.open_n[0] == 2 && dev.njobs() == 4);
    dev.release(dev.job(0));
    wait_for([&] { return dev.njobs() == 5; }, "the leader did not launch");
    s.check_carries(dev.job(4), {a, b}, 0);
    dev.release(dev.job(4));
    s.finish_all_ok();
    check_idle(core);
    CHECK(dev.solo_calls == 4 && counters(core) == (U64s{1, 2}));
}

// ---- 5: a failed combined launch -----------------------------------------------------------------
static void failed_launch() {
    Watchdog wd("a failed combined launch");
    Core core(1, 4);
    FakeDev& dev = core.dev;
    Script s(core, 5);
    s.start_alone(0);
    const size_t a = s.start_joining(0, 1, 16, 100), b = s.start_joining(1, 1, 0, 0), c = s.start_joining(2, 1, 17, 7, 1, kForged);
    dev.fail_combined = 1;
    dev.release(dev.job(0));
    for (size_t k : {a, b, c}) {
        s.join(k);
        CHECK(call_untouched(s.calls[k]));  // NEB_ERR_HIP for every owner, no output written
    }
    s.finish_ok(0);
    check_idle(core);  // inflight is back, the buffer recycled
    CHECK(dev.failed_launches == 1 && dev.njobs() == 1 && core.state().batches == 1);
    // the next calls succeed, on the same buffer
    const size_t t1 = s.start_alone(1);
    const size_t d = s.start_joining(0, 1, 16, 100), e = s.start_joining(1, 1, 1, 1);
    dev.release(dev.job(1));
    wait_for([&] { return dev.njobs() == 3; }, "the leader did not launch");
    s.check_carries(dev.job(2), {d, e}, 1);
    dev.release(dev.job(2));
    for (size_t k : {t1, d, e}) s.finish_ok(k);
    check_idle(core);
    CHECK(core.state().batches == 1 && dev.reserves == 1);
}

// ---- 6: unpublished statuses ---------------------------------------------------------------------
static void unpublished() {
    Watchdog wd("unpublished statuses");
    Core core(1, 4);
    FakeDev& dev = core.dev;
    Script s(core, 6);
    s.start_alone(0);
    s.start_joining(0, 0, 13, 100);
    s.start_joining(1, 0, 0, 0);
    s.start_joining(2, 0, 16, 2032, 8);
    dev.unpublish_combined = 1;
    dev.release(dev.job(0));
    wait_for([&] { return dev.njobs() == 2; }, "the leader did not launch");
    CHECK(!dev.job(1)->publish);
    dev.release(dev.job(1));
    s.finish_all_ok();  // the launch's completion delivered the results
    CHECK(dev.syncs == 1);
    check_idle(core);
}

// ---- run(): a batch of one thread's requests beside a gathering batch ----------------------------
static void direct_run() {
    Watchdog wd("run");
    Core core(1, 4);
    FakeDev& dev = core.dev;
    Script s(core, 8);
    std::mt19937_64 rng(88);
    int32_t st[kCombMax + 1];
    CHECK(core.run(0, nullptr, 0, nullptr) == NEB_OK && core.run(0, nullptr, 1, st) == NEB_ERR_INVALID);
    std::deque<Call> reqs(5);
    std::vector<neb::CombReq> q;
    const size_t ads[5] = {0, 1, 13, 1348, 17}, lens[5] = {2032, 0, 100, 0, 2032 - 32};
    for (int r = 0; r < 5; r++) {
        make_call(reqs[r], rng, NEB_ALG_AESGCM, 1, ads[r], lens[r], r == 2 ? 9 : 2, 50 + r, r == 4 ? kForged : kClean);
        q.push_back(reqs[r].q);
    }
    // a request past the slot, of the other direction or the other algorithm: nothing launched or written
    std::vector<neb::CombReq> bad = q;
    bad[3].open = 0;
    std::fill(st, st + 6, -77);
    CHECK(core.run(1, bad.data(), 5, st) == NEB_ERR_INVALID);
    bad = q;
    bad[4].alg = NEB_ALG_CHACHAPOLY;
    CHECK(core.run(1, bad.data(), 5, st) == NEB_ERR_INVALID);
    bad = q;
    bad[0].in_len++;
    bad[0].pay_len++;
    CHECK(core.run(1, bad.data(), 5, st) == NEB_ERR_INVALID);
    std::vector<neb::CombReq> many(kCombMax + 1, q[1]);
    CHECK(core.run(1, many.data(), kCombMax + 1, st) == NEB_ERR_INVALID);
    CHECK(dev.njobs() == 0 && core.state().batches == 0 && std::all_of(st, st + 6, [](int32_t v) { return v == -77; }));
    for (auto& c : reqs) CHECK(std::all_of(c.out.begin(), c.out.end(), [](uint8_t x) { return x == 0xAA; }));
    // beside a gathering batch: a batch of its own, launched when a slot frees, the other undisturbed
    s.start_alone(0);
    const size_t g0 = s.start_joining(0, 1, 16, 40);
    int rc = -99;
    std::thread runner([&] { rc = core.run(1, q.data(), 5, st); });
    wait_for([&] { return core.state().gathering == 6; }, "run() did not fill its batch");
    CHECK(core.state().open_n[1] == 1 && core.state().batches == 2 && dev.njobs() == 1);
    dev.release(dev.job(0));
    wait_for([&] { return dev.njobs() == 2; }, "no leader launched");
    dev.release(dev.job(1));
    wait_for([&] { return dev.njobs() == 3; }, "the other leader did not launch");
    dev.release(dev.job(2));
    runner.join();
    const FakeDev::Token jr = dev.job(dev.job(1)->n == 5 ? 1 : 2);
    CHECK(jr->n == 5 && jr->open == 1);
    for (uint32_t r = 0; r < 5 && r < jr->n; r++) CHECK(jr->descs[r].counter == 50 + r && jr->descs[r].aad_off == r * (uint64_t)kCombSlot);
    CHECK(rc == NEB_OK);
    for (int r = 0; r < 5; r++) {
        reqs[r].rc = rc;
        reqs[r].st = st[r];
        CHECK(call_ok(reqs[r]));
    }
    CHECK(st[2] == NEB_STATUS_BAD_KEY && st[4] == NEB_STATUS_AUTH_FAILED && st[0] == NEB_STATUS_OK);
    s.finish_all_ok();
    (void)g0;
    check_idle(core);
    CHECK(counters(core) == (U64s{2, 6}));
    // a failed launch: every status and output untouched
    for (auto& c : reqs) std::fill(c.out.begin(), c.out.end(), 0xAA);
    std::fill(st, st + 6, -77);
    dev.fail_combined = 1;
    CHECK(core.run(1, q.data(), 5, st) == NEB_ERR_HIP);
    CHECK(std::all_of(st, st + 6, [](int32_t v) { return v == -77; }));
    for (auto& c : reqs) CHECK(std::all_of(c.out.begin(), c.out.end(), [](uint8_t x) { return x == 0xAA; }));
    check_idle(core);
}

// ---- 7: many threads against random completion order ---------------------------------------------
static void stress() {
    Watchdog wd("many threads");
    Core core(4, 4);
    FakeDev& dev = core.dev;
    dev.unpublish_every = 5;
    constexpr int kThreads = 64, kRounds = 24;
    std::atomic<bool> stop{false};
    std::thread releaser([&] {  // completes the held launches in a random order
        std::mt19937_64 rng(777);
        while (!stop.load()) {
            FakeDev::Token j = dev.pick_unreleased(rng);
            if (j) dev.release(j);
            else std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
    });
    std::atomic<uint64_t> calls{0}, bad{0};
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; t++)
        th.emplace_back([&, t] {
            std::mt19937_64 rng(9000 + t);
            static const size_t ads[] = {0, 1, 13, 16, 17, 48, 1348}, lens[] = {0, 1, 16, 90, 576, 1300};
            for (int r = 0; r < kRounds; r++) {
                const uint64_t ctr = ((uint64_t)t << 32) + (uint64_t)r * 64;
                if (t % 8 == 0) {  // some threads place whole batches (run)
                    const uint32_t n = 1 + rng() % kCombMax;
                    const int open = rng() & 1;
                    std::deque<Call> reqs(n);
                    std::vector<neb::CombReq> q;
                    for (uint32_t k = 0; k < n; k++) {
                        const size_t ad = ads[rng() % 7];
                        make_call(reqs[k], rng, NEB_ALG_AESGCM, open, ad, ad == 1348 ? 0 : lens[rng() % 6],
                                  rng() % 16 ? rng() % kKeys : kKeys + 1, ctr + k, rng() % 8 ? kClean : kForged);
                        q.push_back(reqs[k].q);
                    }
                    std::vector<int32_t> st(n, -77);
                    const int rc = core.run(open, q.data(), n, st.data());
                    for (uint32_t k = 0; k < n; k++) {
                        reqs[k].rc = rc;
                        reqs[k].st = st[k];
                        if (!call_ok(reqs[k])) bad++;
                    }
                    calls += n;
                    continue;
                }
                Call c;
                const size_t ad = ads[rng() % 7];
                const int alg = rng() % 10 ? NEB_ALG_AESGCM : NEB_ALG_CHACHAPOLY;
                const size_t len = rng() % 16 == 0 ? 2100 : ad == 1348 ? 0 : lens[rng() % 6];  // some past the slot
                make_call(c, rng, alg, rng() & 1, ad, len, rng() % 16 ? rng() % kKeys : kKeys + 1, ctr,
                          rng() % 8 ? kClean : kForged);
                c.rc = core.call(c.q, &c.st);
                if (!call_ok(c)) bad++;
                calls++;
            }
        });
    for (auto& x : th) x.join();
    stop = true;
    releaser.join();
    CHECK(bad == 0);
    check_idle(core);
    const U64s c = counters(core);
    size_t combined_jobs = 0;
    for (size_t k = 0; k < dev.njobs(); k++) combined_jobs += dev.job(k)->combined;
    // every call counted once, alone or combined
    CHECK(dev.solo_calls + dev.counted == calls && c[1] == dev.counted && c[0] == combined_jobs);
    CHECK(c[0] > 0 && c[1] <= kCombMax * c[0] && dev.syncs > 0);
}

int main() {
    std::mt19937_64 rng(1);
    for (auto& k : g_keys) k = (uint8_t)rng();
    gathering();
    full_batch();
    directions();
    ineligible();
    failed_launch();
    unpublished();
    direct_run();
    stress();
    std::printf("comb_test: %s\n", fails ? "FAILED" : "ok");
    return fails ? 1 : 0;
}
