// pipe_test.cpp — sanitizer test (ASan + UBSan, and TSan) of the staged host pipeline's pure parts
// (nebula_amd/csrc/pipe_core.hpp) against brute force: the chunk plan, a chunk's arena span with
// its descriptors rebased onto it, and the overlap test between the spans of chunks in flight.
// TEST INFRASTRUCTURE; `make -C tests/sanitize`.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "../../nebula_amd/csrc/host_common.hpp"
#include "../../nebula_amd/csrc/pipe_core.hpp"

static int fails = 0;
#define CHECK(x)                                                                              \
    do {                                                                                      \
        if (!(x)) {                                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x);        \
            fails++;                                                                          \
        }                                                                                     \
    } while (0)

using Plan = std::vector<uint32_t>;
static_assert(neb::kPipeFirst == 4096 && neb::kPipeChunkPkts == 16384 && neb::kPipeSlots == 4,
              "the expected plans below are those of the default tuning");

// The plan as engine.cpp computed it before pipe_core.hpp, written from its description: the ramp
// 4096, 8192 at both ends while four times the next step still fits, full chunks between, the
// remainder last of them. *ramp: the number of chunks in each end's ramp.
static Plan plan_ref(uint32_t n, size_t* ramp) {
    uint32_t rem = n;
    Plan up;
    for (uint32_t s : {4096u, 8192u}) {
        if (rem < 4u * s) break;
        up.push_back(s);
        rem -= 2u * s;
    }
    Plan p = up;
    while (rem > 16384u) {
        p.push_back(16384u);
        rem -= 16384u;
    }
    if (rem) p.push_back(rem);
    for (size_t i = up.size(); i-- > 0;) p.push_back(up[i]);
    *ramp = up.size();
    return p;
}

static void check_plan(uint32_t n) {
    const Plan p = neb::pipe_plan(n);
    size_t ramp = 0;
    CHECK(p == plan_ref(n, &ramp));
    uint64_t sum = 0;
    for (uint32_t c : p) {
        sum += c;
        CHECK(c != 0 && c <= neb::kPipeChunkPkts);
    }
    CHECK(sum == n);
    CHECK(p.size() >= 2 * ramp + 1);
    for (size_t i = 0; i < ramp && 2 * i < p.size(); i++)  // the ramp: a palindrome, doubling from kPipeFirst
        CHECK(p[i] == neb::kPipeFirst << i && p[p.size() - 1 - i] == p[i]);
    for (size_t i = ramp; i + ramp + 1 < p.size(); i++) CHECK(p[i] == neb::kPipeChunkPkts);  // full but the last
}

static void test_plan() {
    for (uint32_t n = 1; n <= 200000; n += 97) check_plan(n);  // 97: coprime to 4096, every residue
    for (uint32_t n : {16383u, 16384u, 16385u, 40959u, 40960u, 65536u}) check_plan(n);
    CHECK(neb::pipe_plan(0).empty());
    CHECK(neb::pipe_plan(16383) == (Plan{16383}));
    CHECK(neb::pipe_plan(16384) == (Plan{4096, 8192, 4096}));
    CHECK(neb::pipe_plan(16385) == (Plan{4096, 8193, 4096}));
    CHECK(neb::pipe_plan(20000) == (Plan{4096, 11808, 4096}));
    CHECK(neb::pipe_plan(40959) == (Plan{4096, 16384, 16383, 4096}));
    // the smallest batch whose fifth chunk takes slot 0 again
    CHECK(neb::pipe_plan(40960) == (Plan{4096, 8192, 16384, 8192, 4096}));
    CHECK(neb::pipe_plan(65536) == (Plan{4096, 8192, 16384, 16384, 8192, 8192, 4096}));
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static void test_span_rebase() {
    for (int round = 0; round < 2000; round++) {
        const int open = round & 1;
        const uint64_t arena_len = 4096 + rnd() % (1u << 20);
        // a window of the arena, so that most chunks' spans start well inside it
        const uint64_t win_lo = rnd() % (arena_len - 2048), win_len = 2048 + rnd() % (arena_len - win_lo - 2047);
        const uint32_t cnt = 1 + (uint32_t)(rnd() % 64);
        std::vector<neb_desc> d(cnt), out(cnt);
        for (auto& x : d) {
            x.len = (uint32_t)(rnd() % 1501);
            x.aad_len = (uint32_t)(rnd() % 65);
            x.src_off = win_lo + rnd() % (win_len - (x.len + 16u) + 1);
            x.dst_off = (rnd() & 1) ? x.src_off : win_lo + rnd() % (win_len - (x.len + 16u) + 1);
            x.aad_off = win_lo + rnd() % (win_len - x.aad_len + 1);
            x.counter = rnd();
            x.key_id = (uint32_t)rnd();
            x.flags = (uint32_t)rnd();
            CHECK(neb_desc_in_arena(x, open, arena_len));
        }
        const neb::PipeSpan sp = neb::pipe_span(d.data(), cnt, open);
        // brute force: the lowest and highest byte any descriptor touches
        uint64_t lo = ~0ull, hi = 0;
        for (const auto& x : d) {
            const uint64_t in = x.len + (open ? 16u : 0u), outl = x.len + (open ? 0u : 16u);
            for (uint64_t o : {x.src_off, x.dst_off, x.aad_off}) lo = o < lo ? o : lo;
            for (uint64_t e : {x.src_off + in, x.dst_off + outl, x.aad_off + x.aad_len}) hi = e > hi ? e : hi;
        }
        CHECK(sp.lo % 16 == 0 && sp.lo <= lo && lo - sp.lo < 16 && sp.hi == hi && sp.hi <= arena_len);
        neb::pipe_rebase(out.data(), d.data(), cnt, sp.lo);
        const uint64_t bytes = sp.hi - sp.lo;
        for (uint32_t i = 0; i < cnt; i++) {
            const neb_desc &x = d[i], &y = out[i];
            CHECK(neb_desc_in_arena(y, open, bytes));  // every range inside [0, hi - lo)
            CHECK(y.src_off == x.src_off - sp.lo && y.dst_off == x.dst_off - sp.lo && y.aad_off == x.aad_off - sp.lo);
            CHECK(y.src_off % 16 == x.src_off % 16 && y.dst_off % 16 == x.dst_off % 16 &&
                  y.aad_off % 16 == x.aad_off % 16);
            CHECK(y.len == x.len && y.aad_len == x.aad_len && y.counter == x.counter && y.key_id == x.key_id &&
                  y.flags == x.flags);
        }
    }
}

static void test_overlap() {
    using S = neb::PipeSpan;
    CHECK(!(S{0, 16}.overlaps(S{16, 32})) && !(S{16, 32}.overlaps(S{0, 16})));  // touching
    CHECK((S{0, 17}.overlaps(S{16, 32})) && (S{16, 32}.overlaps(S{0, 17})));    // one byte shared
    CHECK((S{0, 100}.overlaps(S{16, 32})) && (S{16, 32}.overlaps(S{0, 100})));  // containment
    CHECK((S{16, 32}.overlaps(S{16, 32})));
    for (int round = 0; round < 20000; round++) {
        S a, b;
        a.lo = rnd() % 64, a.hi = a.lo + 1 + rnd() % 32;
        b.lo = rnd() % 64, b.hi = b.lo + 1 + rnd() % 32;
        bool shared = false;  // brute force: some byte lies in both
        for (uint64_t x = a.lo; x < a.hi; x++) shared = shared || (b.lo <= x && x < b.hi);
        CHECK(a.overlaps(b) == shared && b.overlaps(a) == shared);
        CHECK(!(a.overlaps(S{a.hi, a.hi + 1 + rnd() % 32})) && !(S{a.hi, a.hi + 8}.overlaps(a)));
        const S in{a.lo + rnd() % (a.hi - a.lo), a.hi};
        CHECK(a.overlaps(in) && in.overlaps(a));
    }
}

int main() {
    test_plan();
    test_span_rebase();
    test_overlap();
    if (fails) {
        std::fprintf(stderr, "pipe_test: %d check(s) failed\n", fails);
        return 1;
    }
    std::printf("pipe_test: ok\n");
    return 0;
}
