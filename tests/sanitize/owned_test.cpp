// owned_test.cpp — sanitizer test (ASan + UBSan with leak detection, and TSan) of the owned buffer
// (nebula_amd/csrc/hip_owned.hpp) over a fake device that logs every call and aborts on a block
// freed twice or never allocated. The test pins which calls reserve, a move and the destructor
// make and in which order; the leak check covers what the fake allocated.
// TEST INFRASTRUCTURE; `make -C tests/sanitize`.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../nebula_amd/csrc/hip_owned.hpp"

static int fails = 0;
#define CHECK(x)                                                                              \
    do {                                                                                      \
        if (!(x)) {                                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x);        \
            fails++;                                                                          \
        }                                                                                     \
    } while (0)

struct Fake {
    using Error = int;
    static constexpr int kOk = 0;
    static inline std::vector<std::string> log;
    static inline std::set<uint8_t*> live;  // device and pinned blocks alike
    static inline int fail_in = 0;          // 1: the next allocation fails, 2: the one after it, ...

    static int alloc(const char* what, uint8_t** p, size_t bytes) {
        log.push_back(what);
        if (fail_in > 0 && --fail_in == 0) return 2;
        *p = static_cast<uint8_t*>(std::malloc(bytes ? bytes : 1));
        live.insert(*p);
        return kOk;
    }
    static void release(const char* what, uint8_t* p) {
        log.push_back(what);
        if (live.erase(p) != 1) {
            std::fprintf(stderr, "owned_test: %s of a block that is not live\n", what);
            std::abort();
        }
        std::free(p);
    }
    static int mem_alloc(uint8_t** p, size_t bytes) { return alloc("alloc", p, bytes); }
    static void mem_free(uint8_t* p) { release("free", p); }
    static int host_alloc(uint8_t** p, size_t bytes, unsigned flags) {
        return alloc(flags == 2u ? "host_alloc mapped" : "host_alloc", p, bytes);
    }
    static void host_free(uint8_t* p) { release("host_free", p); }
};

using Buf = neb::OwnedBuf<Fake>;
using Pinned = neb::OwnedBuf<Fake, uint32_t, 0>;
using Mapped = neb::OwnedBuf<Fake, uint32_t, 2>;
using Log = std::vector<std::string>;

static Log take() {
    Log l;
    l.swap(Fake::log);
    return l;
}
// the caller's wait, logged
static auto waited = [] {
    Fake::log.push_back("wait");
    return Fake::kOk;
};

static void test_reserve() {
    Buf b;
    bool grew = false;
    CHECK(!b && b.bytes() == 0);
    // nothing to free yet: no wait, one allocation
    CHECK(b.reserve(1000, &grew, waited) == Fake::kOk);
    CHECK((take() == Log{"alloc"}));
    CHECK(grew && b && b.bytes() == 1000);
    // (a) within capacity: no call at all
    uint8_t* p = b;
    CHECK(b.reserve(1000, &grew, waited) == Fake::kOk && !grew);
    CHECK(b.reserve(1, &grew, waited) == Fake::kOk && !grew);
    CHECK(take().empty() && (uint8_t*)b == p && b.bytes() == 1000);
    // (b) growth: the caller's wait, then one free, then one allocation
    CHECK(b.reserve(4096, &grew, waited) == Fake::kOk);
    CHECK((take() == Log{"wait", "free", "alloc"}));
    CHECK(grew && b.bytes() == 4096 && Fake::live.size() == 1);
    // a wait that fails: nothing freed, the buffer as it was
    p = b;
    CHECK(b.reserve(8192, &grew, [] { return 7; }) == 7);
    CHECK(take().empty() && !grew && (uint8_t*)b == p && b.bytes() == 4096);
    // (c) a failed allocation: empty, capacity 0; the next reserve allocates and frees nothing
    Fake::fail_in = 1;
    CHECK(b.reserve(1 << 20, &grew, waited) != Fake::kOk);
    CHECK((take() == Log{"wait", "free", "alloc"}));
    CHECK(!grew && !b && b.bytes() == 0 && Fake::live.empty());
    CHECK(b.reserve(64, &grew, waited) == Fake::kOk);
    CHECK((take() == Log{"alloc"}));
    CHECK(grew && b && b.bytes() == 64);
    // (e) the destructor frees exactly once
}

static void test_move_and_kinds() {
    CHECK((take() == Log{"free"}) && Fake::live.empty());  // test_reserve's buffer
    {
        Pinned a;
        CHECK(a.reserve(16) == Fake::kOk);  // (no wait given: nothing can be using the old block)
        a[0] = 5;
        Pinned b(std::move(a));
        CHECK(!a && a.bytes() == 0 && b && b[0] == 5 && b.bytes() == 16);
        Pinned c;
        CHECK(c.reserve(8) == Fake::kOk);
        CHECK((take() == Log{"host_alloc", "host_alloc"}));
        Mapped m;
        CHECK(m.reserve(8) == Fake::kOk);
        CHECK((take() == Log{"host_alloc mapped"}));
        std::vector<Pinned> v;  // as the engine keeps its receive slots
        v.push_back(std::move(c));
        v.emplace_back();
        v.emplace_back();  // (the vector grows: its elements move again)
        CHECK(!c && v[0].bytes() == 8 && take().empty() && Fake::live.size() == 3);
    }
    // (d) the moved-from buffers freed nothing; (e) each block once
    CHECK((take() == Log{"host_free", "host_free", "host_free"}) && Fake::live.empty());
}

// (f) a slot set up resource by resource, as the staged pipeline's (Pipe::ensure): a failure in the
// middle returns early, and the next call completes the slot
struct Slot {
    Pinned h_desc;
    Buf d_desc;
    Pinned h_status;
    int ensure() {
        int err;
        if ((err = h_desc.reserve(64)) != Fake::kOk) return err;
        if ((err = d_desc.reserve(64)) != Fake::kOk) return err;
        return h_status.reserve(16);
    }
};

static void test_ensure() {
    {
        Slot s;
        Fake::fail_in = 2;  // the second of the three
        CHECK(s.ensure() != Fake::kOk);
        CHECK((take() == Log{"host_alloc", "alloc"}));
        CHECK(s.h_desc && !s.d_desc && !s.h_status);
        CHECK(s.ensure() == Fake::kOk);
        CHECK((take() == Log{"alloc", "host_alloc"}));  // only what was missing
        CHECK(s.h_desc && s.d_desc && s.h_status && Fake::live.size() == 3);
        CHECK(s.ensure() == Fake::kOk && take().empty());  // complete: no call
    }
    CHECK((take() == Log{"host_free", "free", "host_free"}) && Fake::live.empty());
}

int main() {
    test_reserve();
    test_move_and_kinds();
    test_ensure();
    CHECK(Fake::live.empty());
    if (fails) {
        std::fprintf(stderr, "owned_test: %d failures\n", fails);
        return 1;
    }
    std::printf("owned_test: ok\n");
    return 0;
}
