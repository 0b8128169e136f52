// window_test.cpp — sanitizer test (ASan + UBSan, and TSan) of the host receive logic in
// nebula_amd/csrc/window_core.hpp: Nebula's replay window (WindowCore, bits.go:15-262), the exact
// receive order over window runs (exact_rounds), the host receive's steps before it, the layout of
// the speculative arena and the thread pool the batched receive spreads windows over (RxPool).
// TEST INFRASTRUCTURE; built and run by `make -C tests/sanitize`.
//
//  1. random Check/Update streams over every window length 1..8192, counters near 0 and near 2^64
//     (clear_range's circular slot arithmetic, the warmup path, jumps past the window);
//  2. exact_rounds over many windows with forged packets, against the packet-by-packet loop
//     (connection_state.go:99-119): statuses, commits and window states must match, with the
//     per-window groups spread over an RxPool and several threads running batches at once;
//  3. the host receive's own steps in the order window.cpp takes them (group_by_window,
//     split_windows, simulate_admits, compact_admitted, exact_rounds) with a fake verifier, against
//     the same loop: windows of several lengths with prior state, packets whose key names no window;
//  4. spec_layout over every pair of edge AAD and payload lengths: aligned, disjoint copies inside
//     the reported size that reproduce every packet's bytes;
//  5. RxPool::run from several threads at once.
#include <cassert>
#include <cinttypes>
#include <cstdio>
#include <random>

#include "../../nebula_amd/csrc/window_core.hpp"

using namespace neb_rx;

static WindowCore make_window(uint64_t length) {
    WindowCore w;
    w.length = length;
    w.mask = length - 1;
    w.words.assign(length >= 64 ? length / 64 : 1, 0);
    w.words[0] = 1;  // counter 0 seeded as received (bits.go:47-48)
    return w;
}

static bool same(const WindowCore& a, const WindowCore& b) {
    return a.current == b.current && a.words == b.words && a.lost == b.lost && a.dupe == b.dupe &&
           a.out_of_window == b.out_of_window;
}

static int fails = 0;
#define CHECK(x)                                                                 \
    do {                                                                         \
        if (!(x)) {                                                              \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
            fails++;                                                             \
        }                                                                        \
    } while (0)

static void random_streams() {
    std::mt19937_64 rng(7);
    for (uint64_t len = 1; len <= 8192; len <<= 1) {
        for (int base_kind = 0; base_kind < 3; base_kind++) {
            WindowCore w = make_window(len);
            uint64_t base = base_kind == 0 ? 0 : base_kind == 1 ? (1ull << 62) : ~0ull - 20000;
            if (base) w.update(base);
            for (int k = 0; k < 1000; k++) {
                const uint64_t r = rng();
                uint64_t c;
                switch (r % 5) {
                    case 0: c = w.current + 1; break;
                    case 1: c = w.current - (r >> 8) % (2 * len + 3); break;
                    case 2: c = w.current + (r >> 8) % (3 * len + 5); break;
                    case 3: c = w.current + (r >> 8) % 4; break;
                    default: c = (r >> 3) % 4 == 0 ? ~0ull - (r >> 8) % 64 : w.current + 2; break;
                }
                const uint64_t before = w.current;
                const bool ok = w.check(c);
                const bool up = w.update(c);
                // an update never accepts what check refused on the same state, except Go's uint64
                // wrap at the top of the counter space (i == current + 1 == 0, bits.go:171)
                CHECK(!up || ok || before == ~0ull);
            }
        }
    }
}

struct Pkt {
    uint32_t w;
    uint64_t c;
    bool forged;
};

// the packet-by-packet receive (connection_state.go:99-119) over private copies of the windows
static void sequential(std::vector<WindowCore>& wins, const std::vector<Pkt>& pk, std::vector<int32_t>& st) {
    for (size_t i = 0; i < pk.size(); i++) {
        WindowCore& w = wins[pk[i].w];
        if (!w.check(pk[i].c)) {
            st[i] = NEB_STATUS_REPLAY;
            continue;
        }
        if (pk[i].forged) {
            st[i] = NEB_STATUS_AUTH_FAILED;
            continue;
        }
        st[i] = w.update(pk[i].c) ? NEB_STATUS_OK : NEB_STATUS_REPLAY;
    }
}

// exact_rounds over the same batch, starting from nothing opened (every packet held back)
static void exact(std::vector<WindowCore>& wins, std::vector<std::mutex>& mus, const std::vector<Pkt>& pk,
                  std::vector<int32_t>& st, RxPool& pool, uint32_t groups, uint32_t* opens) {
    const uint32_t n = (uint32_t)pk.size(), nw = (uint32_t)wins.size();
    std::vector<uint32_t> order;
    std::vector<ExactRun> runs;
    for (uint32_t w = 0; w < nw; w++) {
        const uint32_t k0 = (uint32_t)order.size();
        for (uint32_t i = 0; i < n; i++)
            if (pk[i].w == w) order.push_back(i);
        if (order.size() > k0) runs.push_back({w, k0, (uint32_t)order.size()});
    }
    std::vector<uint8_t> opened(n, 0);
    std::vector<int32_t> verd(n, NEB_STATUS_BAD_KEY);
    std::vector<uint32_t> commit, zero;
    auto verify = [&](const std::vector<uint32_t>& p, uint8_t how) {
        for (uint32_t i : p) {
            CHECK(!opened[i]);
            opened[i] = how;
            verd[i] = pk[i].forged ? NEB_STATUS_AUTH_FAILED : NEB_STATUS_OK;
        }
        (*opens)++;
        return NEB_OK;
    };
    const int rc = exact_rounds(
        runs, groups, [&](uint32_t k) { return pk[order[k]].c; }, [&](uint32_t k) { return order[k]; },
        opened.data(), verd.data(), st.data(),
        [&](uint32_t w, auto&& fn) {
            std::lock_guard<std::mutex> g(mus[w]);
            fn(wins[w]);
        },
        [&](const std::vector<uint32_t>& p) { return verify(p, 1); },
        [&](const std::vector<uint32_t>& p) { return verify(p, 2); },
        [&](uint32_t cnt, auto&& fn) { pool.run(cnt, fn); }, &commit, &zero);
    CHECK(rc == NEB_OK);
    for (uint32_t i : commit) CHECK(opened[i] == 2 && st[i] == NEB_STATUS_OK);
    for (uint32_t i : zero) CHECK(opened[i] == 2 && st[i] == NEB_STATUS_AUTH_FAILED);
}

static void exact_vs_sequential(uint64_t seed, RxPool& pool) {
    std::mt19937_64 rng(seed);
    const uint32_t nw = 1 + rng() % 40;
    const uint64_t len = 1ull << (rng() % 11);
    std::vector<Pkt> pk;
    std::vector<uint64_t> cur(nw, 2);
    for (int i = 0; i < 4000; i++) {
        const uint32_t w = rng() % nw;
        const uint64_t r = rng();
        uint64_t c;
        if (r % 100 < 4) c = cur[w] + 100000 + r % 1000000;  // a forged far-ahead counter
        else if (r % 100 < 70) c = ++cur[w];
        else c = cur[w] - r % (len + 4) + 1;
        pk.push_back({w, c, r % 100 < 4 || (r >> 20) % 50 == 0});
    }
    std::vector<WindowCore> a, b;
    for (uint32_t w = 0; w < nw; w++) {
        a.push_back(make_window(len));
        a.back().update(1);
        a.back().update(2);
    }
    b = a;
    std::vector<std::mutex> mus(nw);
    std::vector<int32_t> sa(pk.size(), -1), sb(pk.size(), -1);
    sequential(a, pk, sa);
    uint32_t opens = 0;
    exact(b, mus, pk, sb, pool, 4, &opens);
    CHECK(sa == sb);
    for (uint32_t w = 0; w < nw; w++) CHECK(same(a[w], b[w]));
    CHECK(opens <= 3);  // the simulation's batch, then at most one in-place and one speculative round
}

// The host receive as window.cpp runs it, the GPU replaced by the packets' forged flags.
static void steps_vs_sequential(uint64_t seed, RxPool& pool, uint32_t groups) {
    std::mt19937_64 rng(seed);
    const uint32_t nw = 1 + rng() % 40, n = 4000;
    std::vector<WindowCore> a, b;
    std::vector<uint8_t> present(nw);  // 0: a null window pointer
    std::vector<uint64_t> cur(nw, 0);
    for (uint32_t w = 0; w < nw; w++) {
        a.push_back(make_window(1ull << (rng() % 11)));
        for (uint32_t j = rng() % 40; j > 0; j--) a.back().update(cur[w] += 1 + rng() % 3);  // prior state
        present[w] = rng() % 8 != 0;
    }
    b = a;
    std::vector<neb_desc> desc(n, neb_desc{});
    std::vector<uint8_t> forged(n);
    std::vector<Pkt> seq;  // the packets that have a window, for sequential()
    std::vector<uint32_t> seq_i;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t w = rng() % nw;
        const uint64_t r = rng();
        uint64_t c;
        if (r % 100 < 4) c = cur[w] + 100000 + r % 1000000;  // a forged far-ahead counter
        else if (r % 100 < 70) c = ++cur[w];
        else c = cur[w] - r % (a[w].length + 4) + 1;  // a replay, inside or behind the window
        forged[i] = r % 100 < 4 || (r >> 20) % 50 == 0;
        desc[i].counter = c;
        desc[i].len = i;  // (names the packet in the compacted copy)
        desc[i].key_id = (r >> 40) % 64 == 0 ? nw + (uint32_t)(r >> 50) % 3 : w;  // past every window
        if (desc[i].key_id < nw && present[w]) {
            seq.push_back({w, c, (bool)forged[i]});
            seq_i.push_back(i);
        }
    }
    std::vector<int32_t> want(n, NEB_STATUS_BAD_KEY), seq_st(seq.size(), -1), st(n, -1);
    sequential(a, seq, seq_st);
    for (size_t j = 0; j < seq.size(); j++) want[seq_i[j]] = seq_st[j];

    auto group_of = [&](uint32_t i) { return desc[i].key_id < nw && present[desc[i].key_id] ? desc[i].key_id : nw; };
    const RxGroups G = group_by_window(
        n, nw, [&](uint32_t i) { return desc[i].key_id; }, [&](uint32_t g) { return present[g] != 0; });
    CHECK(G.start.size() == nw + 2 && G.start[0] == 0 && G.start[nw + 1] == n && G.order.size() == n);
    for (uint32_t g = 0; g <= nw; g++)
        for (uint32_t k = G.start[g]; k < G.start[g + 1]; k++) {
            CHECK(group_of(G.order[k]) == g);
            CHECK(k == G.start[g] || G.order[k - 1] < G.order[k]);  // arrival order inside the window
        }
    const std::vector<uint32_t> wsplit = split_windows(G.start, nw, groups);
    CHECK(wsplit.size() == groups + 1 && wsplit[0] == 0 && wsplit[groups] == nw);
    for (uint32_t t = 0; t < groups; t++) CHECK(wsplit[t] <= wsplit[t + 1]);

    std::vector<std::mutex> mus(nw);
    auto with_window = [&](uint32_t w, auto&& fn) {
        std::lock_guard<std::mutex> g(mus[w]);
        fn(b[w]);
    };
    auto par = [&](uint32_t cnt, auto&& fn) { pool.run(cnt, fn); };
    std::vector<uint8_t> opened = simulate_admits(G, wsplit, [&](uint32_t i) { return desc[i].counter; }, with_window, par);
    std::vector<uint8_t> brute(n, 0);  // the same question asked packet by packet
    std::vector<WindowCore> sim = b;
    for (uint32_t i = 0; i < n; i++)
        if (group_of(i) < nw && sim[group_of(i)].check(desc[i].counter)) {
            sim[group_of(i)].update(desc[i].counter);
            brute[i] = 1;
        }
    CHECK(opened == brute);
    for (uint32_t w = 0; w < nw; w++) CHECK(same(b[w], a[w]) || present[w]);  // (no window moved yet)

    std::vector<uint32_t> sub_of(n, ~0u);
    std::vector<neb_desc> sub;
    const uint32_t m = compact_admitted(desc.data(), opened.data(), n, sub_of.data(), [&](uint32_t cnt) {
        sub.assign(cnt, neb_desc{});
        return sub.data();
    });
    uint32_t j = 0;
    for (uint32_t i = 0; i < n; i++)
        if (opened[i]) {
            CHECK(sub_of[i] == j && j < m && sub[j].len == i && sub[j].counter == desc[i].counter);
            j++;
        }
    CHECK(j == m && sub.size() == m);

    uint32_t opens = 0;
    std::vector<int32_t> verd(n, NEB_STATUS_BAD_KEY);
    if (m) opens++;  // the plan's batch, verdicts by compacted position
    for (uint32_t i = 0; i < n; i++)
        if (opened[i]) verd[i] = forged[sub[sub_of[i]].len] ? NEB_STATUS_AUTH_FAILED : NEB_STATUS_OK;
    auto verify = [&](const std::vector<uint32_t>& p, uint8_t how) {
        for (uint32_t i : p) {
            CHECK(!opened[i]);
            opened[i] = how;
            verd[i] = forged[i] ? NEB_STATUS_AUTH_FAILED : NEB_STATUS_OK;
        }
        opens++;
        return NEB_OK;
    };
    for (uint32_t k = G.start[nw]; k < G.start[nw + 1]; k++) st[G.order[k]] = NEB_STATUS_BAD_KEY;
    std::vector<uint32_t> commit, zero;
    const int rc = exact_rounds(
        window_runs(G, nw), groups, [&](uint32_t k) { return desc[G.order[k]].counter; },
        [&](uint32_t k) { return G.order[k]; }, opened.data(), verd.data(), st.data(), with_window,
        [&](const std::vector<uint32_t>& p) { return verify(p, 1); },
        [&](const std::vector<uint32_t>& p) { return verify(p, 2); }, par, &commit, &zero);
    CHECK(rc == NEB_OK);
    CHECK(st == want);
    for (uint32_t w = 0; w < nw; w++) CHECK(same(a[w], b[w]));
    CHECK(opens <= 3);  // the plan's batch; exact_rounds adds at most one in-place and one speculative round
}

// every packet admitted: the compaction is one copy
static void compact_all_admitted() {
    std::vector<neb_desc> desc(5, neb_desc{}), out(5, neb_desc{});
    for (uint32_t i = 0; i < 5; i++) desc[i].len = 10 + i;
    const std::vector<uint8_t> plan(5, 1);
    std::vector<uint32_t> sub_of(5, ~0u);
    CHECK(compact_admitted(desc.data(), plan.data(), 5, sub_of.data(), [&](uint32_t) { return out.data(); }) == 5);
    for (uint32_t i = 0; i < 5; i++) CHECK(sub_of[i] == i && out[i].len == 10 + i);
}

static void spec_layout_cases() {
    std::mt19937_64 rng(99);
    const uint32_t aads[6] = {0, 1, 15, 16, 17, 48}, pays[6] = {0, 1, 15, 16, 17, 1300};
    struct Copy {
        uint64_t src, dst, len;
    };
    for (uint32_t batch : {1u, 2u, 37u})
        for (uint32_t pair = 0; pair < 36; pair++) {
            // packet 0 has this pair of lengths, the packets after it the pairs after it; each one's AAD
            // and payload + tag somewhere in a random source arena, at any alignment
            std::vector<neb_desc> desc(batch, neb_desc{});
            uint64_t at = rng() % 16;
            for (uint32_t i = 0; i < batch; i++) {
                neb_desc& d = desc[i];
                d.aad_len = aads[(pair + i) % 36 / 6];
                d.len = pays[(pair + i) % 6];
                d.counter = rng();
                d.key_id = i;
                d.src_off = at;
                d.dst_off = at += d.len + 16 + rng() % 8;  // (a receive may open out of place)
                d.aad_off = at += d.len + rng() % 8;
                at += d.aad_len + rng() % 8;
            }
            std::vector<uint8_t> src(at);
            for (uint8_t& x : src) x = (uint8_t)rng();
            std::vector<uint32_t> pk(batch);
            for (uint32_t i = 0; i < batch; i++) pk[i] = i;
            std::shuffle(pk.begin(), pk.end(), rng);
            std::vector<neb_desc> out(batch);
            std::vector<uint64_t> pt_at(batch, ~0ull);
            std::vector<Copy> copies;
            const uint64_t size = spec_layout(
                pk, [&](uint32_t i) -> const neb_desc& { return desc[i]; }, out.data(), pt_at.data(),
                [&](uint64_t s, uint64_t d, uint64_t l) { copies.push_back({s, d, l}); });
            CHECK(copies.size() == 2 * batch);
            std::vector<uint8_t> spec(size, 0), used(size, 0);
            for (const Copy& c : copies) {
                CHECK(c.dst % 16 == 0 && c.dst <= size && c.len <= size - c.dst);
                CHECK(c.src <= src.size() && c.len <= src.size() - c.src);
                for (uint64_t x = c.dst; x < c.dst + c.len; x++) CHECK(!used[x]++);  // destinations do not overlap
                std::memcpy(spec.data() + c.dst, src.data() + c.src, c.len);
            }
            for (uint32_t j = 0; j < batch; j++) {
                const neb_desc &d = desc[pk[j]], &r = out[j];
                CHECK(r.len == d.len && r.aad_len == d.aad_len && r.counter == d.counter && r.key_id == d.key_id);
                CHECK(r.src_off == r.dst_off && pt_at[pk[j]] == r.dst_off);
                CHECK(r.aad_off + r.aad_len <= size && r.src_off + r.len + 16 <= size);
                CHECK(!std::memcmp(spec.data() + r.aad_off, src.data() + d.aad_off, d.aad_len));
                CHECK(!std::memcmp(spec.data() + r.src_off, src.data() + d.src_off, (size_t)d.len + 16));
            }
        }
}

int main() {
    random_streams();
    compact_all_admitted();
    spec_layout_cases();
    RxPool pool(4);
    std::vector<std::thread> th;
    for (int t = 0; t < 4; t++)
        th.emplace_back([t, &pool] {
            for (int k = 0; k < 6; k++) exact_vs_sequential(1000 * t + k, pool);
            for (int k = 0; k < 3; k++)
                for (uint32_t groups : {1u, 4u}) steps_vs_sequential(5000 * t + k, pool, groups);
        });
    for (auto& x : th) x.join();
    std::atomic<uint64_t> sum{0};
    std::vector<std::thread> runners;
    for (int t = 0; t < 4; t++)
        runners.emplace_back([&] {
            for (int k = 0; k < 50; k++) pool.run(16, [&](uint32_t j) { sum += j; });
        });
    for (auto& x : runners) x.join();
    CHECK(sum == 4ull * 50 * 120);
    std::printf("window_test: %s\n", fails ? "FAILED" : "ok");
    return fails ? 1 : 0;
}
