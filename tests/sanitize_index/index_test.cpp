// index_test.cpp — index_core.hpp and the host table / host form (nebula_amd/csrc/index.cpp) under
// sanitizers: a stand-alone program, no HIP and no GPU.
//   exact    (the ASan + UBSan build) random updates against a std::map, and the host resolve of
//            packets that each live in a heap buffer of exactly their length, with exact-size
//            record arrays: an over-read or a stray write is an ASan report. Then del + put +
//            re-put sequences over the same keys, up to and across the rebuild threshold, against
//            a model that finds its records by linear scan: every key's slot and probe count.
//   threads  (the TSan build) four threads call neb_index_table_update — puts, replaces and deletes
//            of their own churn keys, replaces of the shared steady keys with the same record,
//            through many rebuilds — while two threads run the host resolve: a steady key always
//            resolves to its record, a churn key to its record or to a miss.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "../../nebula_amd/csrc/index_core.hpp"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::abort();                                             \
        }                                                             \
    } while (0)

using Key = std::pair<uint32_t, uint32_t>;  // space, index
using Model = std::map<Key, neb_index_entry>;

static void put_header(uint8_t* h, uint8_t typ, uint8_t sub, uint32_t index) {
    std::memset(h, 0, 16);
    h[0] = (uint8_t)(0x10 | typ);
    h[1] = sub;
    h[4] = (uint8_t)(index >> 24);
    h[5] = (uint8_t)(index >> 16);
    h[6] = (uint8_t)(index >> 8);
    h[7] = (uint8_t)index;
}

static neb_index_entry entry(uint32_t space, uint32_t index, uint32_t key, uint32_t flags, uint32_t tunnel, uint32_t ri) {
    neb_index_entry e{};
    e.index = index;
    e.space = space;
    e.key_id = key;
    e.flags = flags;
    e.route = neb_relay_route{tunnel, ri};
    return e;
}

static const neb_index_entry* lookup(const Model& m, const uint8_t* h, bool* relay) {
    *relay = (h[0] & 15) == 1 && h[1] == 1;
    const uint32_t idx = ((uint32_t)h[4] << 24) | ((uint32_t)h[5] << 16) | ((uint32_t)h[6] << 8) | h[7];
    auto it = m.find(Key{*relay ? 1u : 0u, idx});
    return it == m.end() ? nullptr : &it->second;
}

static void exact() {
    std::mt19937 rng(777);
    neb_index_table* t = nullptr;
    CHECK(neb_index_table_create(nullptr, 8, &t) == NEB_OK);
    const neb_cidr nets[2] = {{{10, 1, 0, 0}, 4, 16, {0, 0}}, {{0xfd, 0, 0, 1}, 6, 32, {0, 0}}};
    CHECK(neb_index_table_set_own_networks(t, nets, 2, nullptr) == NEB_OK);
    Model m;
    const uint32_t pool[12] = {1, 2, 3, 0x80000000u, 0xFFFFFFFFu, 17, 33, 49, 65, 81, 97, 113};
    for (int round = 0; round < 600; round++) {
        // one update: up to two deletions, up to two puts
        std::vector<neb_index_key> del(rng() % 3);
        std::vector<neb_index_entry> put(rng() % 3);
        for (auto& d : del) d = neb_index_key{pool[rng() % 12], (uint32_t)(rng() % 2)};
        for (auto& p : put) {
            const uint32_t space = rng() % 2;
            p = entry(space, pool[rng() % 12], rng() % 5 ? rng() % 64 : NEB_KEYS_MIXED, space ? rng() % 2 : 0,
                      space && rng() % 2 ? rng() % 8 : NEB_RELAY_NONE, rng());
        }
        Model after = m;
        for (auto& d : del) after.erase(Key{d.space, d.index});
        for (auto& p : put) after[Key{p.space, p.index}] = p;
        const int rc = neb_index_table_update(t, del.data(), (uint32_t)del.size(), put.data(), (uint32_t)put.size(), nullptr);
        if (after.size() > 8) {
            CHECK(rc == NEB_ERR_NO_KEY_SLOT);
        } else {
            CHECK(rc == NEB_OK);
            m = after;
        }
        uint32_t live = 0;
        CHECK(neb_index_table_count(t, &live) == NEB_OK && live == m.size());

        // one packet of every length 0..64 and a long one, each alone in a buffer of its length
        const uint32_t len = round % 66 == 65 ? 1364 : round % 66;
        std::vector<uint8_t> arena(len);
        for (auto& b : arena) b = (uint8_t)rng();
        if (len >= 16) put_header(arena.data(), rng() % 4 ? 1 : rng() % 8, rng() % 3, pool[rng() % 12]);
        if (len >= 32) put_header(arena.data() + 16, 1, rng() % 2, pool[rng() % 12]);
        std::vector<neb_rx_packet> pk(1);
        const bool preset = rng() % 4 == 0;
        pk[0] = neb_rx_packet{0, len | (preset ? NEB_RX_OWN_SOURCE : 0u), 0x12345678u};
        std::vector<neb_rx_source> src(1);
        std::memset(&src[0], 0, sizeof src[0]);
        const int kind = rng() % 5;  // none, v4 in, v4 out, v6 in, 4-in-6
        const uint8_t a4in[4] = {10, 1, 9, 9}, a4out[4] = {10, 2, 9, 9}, a6in[16] = {0xfd, 0, 0, 1, 5},
                      a46[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xff, 0xff, 10, 1, 9, 9};
        if (kind == 0) std::memcpy(src[0].addr, a4in, 4);  // family 0: ignored
        if (kind == 1) std::memcpy(src[0].addr, a4in, 4), src[0].family = 4;
        if (kind == 2) std::memcpy(src[0].addr, a4out, 4), src[0].family = 4;
        if (kind == 3) std::memcpy(src[0].addr, a6in, 16), src[0].family = 6;
        if (kind == 4) std::memcpy(src[0].addr, a46, 16), src[0].family = 6;
        std::vector<neb_relay_route> route(1);
        std::vector<neb_rx_via> via(1);
        const bool with_src = rng() % 4 != 0;
        CHECK(neb_rx_resolve_batch_host(t, pk.data(), with_src ? src.data() : nullptr, 1, arena.data(), arena.size(),
                                        rng() % 4 ? route.data() : nullptr, via.data()) == NEB_OK);
        uint32_t key = NEB_KEYS_MIXED;
        neb_rx_via v{NEB_KEYS_MIXED, 0};
        if (len >= 16) {
            bool relay, inner_relay;
            const neb_index_entry* e = lookup(m, arena.data(), &relay);
            if (e) {
                key = e->key_id;
                if (relay && (e->flags & NEB_VIA_TERMINAL)) {
                    v.flags = NEB_VIA_TERMINAL;
                    const neb_index_entry* in = len >= 48 ? lookup(m, arena.data() + 16, &inner_relay) : nullptr;
                    if (in) v.key_id = in->key_id;
                }
            }
        }
        CHECK(pk[0].key_id == key && pk[0].off == 0 && via[0].key_id == v.key_id && via[0].flags == v.flags);
        const bool own = preset || (with_src && (kind == 1 || kind == 3));
        CHECK(pk[0].len == (len | (own ? NEB_RX_OWN_SOURCE : 0u)));
        // an arena one byte short is refused, and nothing is written
        if (len) {
            pk[0].key_id = 5;
            CHECK(neb_rx_resolve_batch_host(t, pk.data(), nullptr, 1, arena.data(), arena.size() - 1, nullptr, via.data()) ==
                  NEB_ERR_INVALID);
            CHECK(pk[0].key_id == 5);
        }
    }
    CHECK(neb_index_table_destroy(t) == NEB_OK);
}

// The table's slot discipline restated with linear scans: a record is found by looking at every
// slot; a put goes to the first EMPTY slot from the key's home, behind the record it replaces, which
// is tombstoned afterwards; past 3/4 of the slots in use the live records are re-inserted in tag order.
struct SlotModel {
    std::vector<uint64_t> tag;  // 0: EMPTY, 1: TOMBSTONE
    std::vector<uint32_t> key;  // the record's key_id
    uint32_t used = 0;
    explicit SlotModel(uint32_t capacity) : tag(neb::idx_slots_for(capacity), 0), key(tag.size(), 0) {}
    int scan(uint64_t want) const {
        for (size_t s = 0; s < tag.size(); s++)
            if (tag[s] == want) return (int)s;
        return -1;
    }
    void insert(uint64_t t, uint32_t space, uint32_t index, uint32_t key_id) {
        size_t s = neb::idx_hash(space, index) % tag.size();
        while (tag[s] != 0) s = (s + 1) % tag.size();
        tag[s] = t;
        key[s] = key_id;
        used++;
    }
    bool update(const std::vector<neb_index_key>& del, const std::vector<neb_index_entry>& put) {  // true: it rebuilt
        if ((uint64_t)used + put.size() > tag.size() / 4 * 3) {
            std::map<uint64_t, uint32_t> recs;
            for (size_t s = 0; s < tag.size(); s++)
                if (tag[s] > 1) recs[tag[s]] = key[s];
            for (auto& d : del) recs.erase(neb::idx_tag(d.space, d.index));
            for (auto& p : put) recs[neb::idx_tag(p.space, p.index)] = p.key_id;
            std::fill(tag.begin(), tag.end(), 0);
            used = 0;
            for (auto& r : recs) insert(r.first, (uint32_t)(r.first >> 32) & 1u, (uint32_t)r.first, r.second);
            return true;
        }
        for (auto& d : del) {
            const int s = scan(neb::idx_tag(d.space, d.index));
            if (s >= 0) tag[(size_t)s] = 1;
        }
        for (auto& p : put) {
            const int old = scan(neb::idx_tag(p.space, p.index));
            insert(neb::idx_tag(p.space, p.index), p.space, p.index, p.key_id);
            if (old >= 0) tag[(size_t)old] = 1;
        }
        return false;
    }
    // what neb_index_table_probe answers: found, the slot the walk ended at, slots examined
    void probe(uint32_t space, uint32_t index, uint32_t out[3]) const {
        const uint64_t want = neb::idx_tag(space, index);
        size_t s = neb::idx_hash(space, index) % tag.size();
        uint32_t k = 1;
        while (tag[s] != want && tag[s] != 0) s = (s + 1) % tag.size(), k++;
        out[0] = tag[s] == want, out[1] = (uint32_t)s, out[2] = k;
    }
};

// del + put + re-put of the same keys in one call, again and again, until live + tombstones + puts
// is exactly `last` of the 32 slots' threshold of 24: at 24 the call still goes slot by slot, at 25
// it rebuilds.
static void exact_slots(uint32_t last) {
    neb_index_table* t = nullptr;
    CHECK(neb_index_table_create(nullptr, 8, &t) == NEB_OK);
    SlotModel m(8);
    CHECK(m.tag.size() == 32);
    const uint32_t idx[5] = {7, 39, 0x80000007u, 71, 1000};  // the last is never put
    uint32_t next_key = 1;
    auto step = [&](uint32_t nput) {
        // deletes the first two keys, puts the first again, then others, then the first once more
        std::vector<neb_index_key> del = {neb_index_key{idx[0], 0}, neb_index_key{idx[1], 1}};
        std::vector<neb_index_entry> put;
        for (uint32_t i = 0; i + 1 < nput; i++) put.push_back(entry(i & 1, idx[i % 4], next_key++, 0, NEB_RELAY_NONE, 0));
        put.push_back(entry(0, idx[0], next_key++, 0, NEB_RELAY_NONE, 0));
        CHECK(neb_index_table_update(t, del.data(), 2, put.data(), nput, nullptr) == NEB_OK);
        const bool rebuilt = m.update(del, put);
        uint32_t live = 0, want_live = 0;
        for (uint64_t tg : m.tag) want_live += tg > 1;
        CHECK(neb_index_table_count(t, &live) == NEB_OK && live == want_live);
        for (uint32_t space = 0; space < 2; space++)
            for (uint32_t index : idx) {
                uint32_t got[3], want[3];
                CHECK(neb_index_table_probe(t, space, index, got) == NEB_OK);
                m.probe(space, index, want);
                CHECK(got[0] == want[0] && got[1] == want[1] && got[2] == want[2]);
                uint8_t h[16];
                put_header(h, 1, (uint8_t)space, index);
                neb_rx_packet pk{0, 16, 0};
                CHECK(neb_rx_resolve_batch_host(t, &pk, nullptr, 1, h, 16, nullptr, nullptr) == NEB_OK);
                CHECK(pk.key_id == (want[0] ? m.key[want[1]] : NEB_KEYS_MIXED));
            }
        return rebuilt;
    };
    while (m.used + 6 <= last) CHECK(!step(3));
    CHECK(m.used == 21);
    const uint32_t before = m.used;
    const bool rebuilt = step(last - before);
    CHECK(rebuilt == (last > 24));
    if (rebuilt) CHECK(m.used <= 4);  // the live records alone
    else CHECK(m.used == 24);         // tombstones and all
    CHECK(step(3) == !rebuilt);       // and the call after it, on the other side
    CHECK(neb_index_table_destroy(t) == NEB_OK);
}

static void threads() {
    constexpr uint32_t kSteady = 16, kChurn = 4, kUpdaters = 4, kRounds = 3000;
    neb_index_table* t = nullptr;
    CHECK(neb_index_table_create(nullptr, kSteady + kUpdaters * kChurn, &t) == NEB_OK);
    std::vector<neb_index_entry> steady;
    for (uint32_t k = 0; k < kSteady; k++) steady.push_back(entry(k & 1, 1000 + k, 100 + k, k & 1, k & 1 ? k : NEB_RELAY_NONE, k));
    CHECK(neb_index_table_update(t, nullptr, 0, steady.data(), kSteady, nullptr) == NEB_OK);
    auto churn = [](uint32_t u, uint32_t k) { return entry(0, 5000 + u * 16 + k, 200 + u * 16 + k, 0, NEB_RELAY_NONE, 0); };
    std::atomic<uint32_t> running{kUpdaters};
    std::vector<std::thread> th;
    for (uint32_t u = 0; u < kUpdaters; u++)
        th.emplace_back([&, u] {
            std::mt19937 rng(u + 1);
            for (uint32_t r = 0; r < kRounds; r++) {
                const neb_index_entry c = churn(u, rng() % kChurn), s = steady[rng() % kSteady];
                const neb_index_key d{c.index, c.space};
                const neb_index_entry put[2] = {s, c};  // the steady key: replaced by the same record
                if (rng() % 2) CHECK(neb_index_table_update(t, nullptr, 0, put, 2, nullptr) == NEB_OK);
                else CHECK(neb_index_table_update(t, &d, 1, put, 1, nullptr) == NEB_OK);
            }
            running--;
        });
    for (uint32_t w = 0; w < 2; w++)
        th.emplace_back([&] {
            const uint32_t n = kSteady + kUpdaters * kChurn;
            std::vector<uint8_t> arena((size_t)n * 16);
            std::vector<neb_index_entry> want;
            for (uint32_t k = 0; k < kSteady; k++) want.push_back(steady[k]);
            for (uint32_t u = 0; u < kUpdaters; u++)
                for (uint32_t k = 0; k < kChurn; k++) want.push_back(churn(u, k));
            std::vector<neb_rx_packet> pk(n);
            std::vector<neb_relay_route> route(n);
            std::vector<neb_rx_via> via(n);
            for (uint32_t i = 0; i < n; i++) put_header(&arena[(size_t)i * 16], 1, (uint8_t)want[i].space, want[i].index);
            uint32_t passes = 0;
            while (running.load() || passes < 3) {
                passes++;
                for (uint32_t i = 0; i < n; i++) pk[i] = neb_rx_packet{(uint64_t)i * 16, 16, 0};
                CHECK(neb_rx_resolve_batch_host(t, pk.data(), nullptr, n, arena.data(), arena.size(), route.data(), via.data()) ==
                      NEB_OK);
                for (uint32_t i = 0; i < n; i++) {
                    const neb_index_entry& e = want[i];
                    const bool hit = pk[i].key_id == e.key_id && route[i].tunnel == e.route.tunnel &&
                                     route[i].remote_index == (e.route.tunnel == NEB_RELAY_NONE ? 0u : e.route.remote_index) &&
                                     via[i].flags == e.flags;
                    const bool miss = pk[i].key_id == NEB_KEYS_MIXED && route[i].tunnel == NEB_RELAY_NONE && via[i].flags == 0;
                    CHECK(hit || (i >= kSteady && miss));  // the steady-key invariant
                }
            }
        });
    for (auto& x : th) x.join();
    uint32_t live = 0;
    CHECK(neb_index_table_count(t, &live) == NEB_OK && live >= kSteady && live <= kSteady + kUpdaters * kChurn);
    CHECK(neb_index_table_destroy(t) == NEB_OK);
}

int main(int argc, char** argv) {
    const bool both = argc < 2;
    if (both || !std::strcmp(argv[1], "exact")) {
        exact();
        exact_slots(24);
        exact_slots(25);
    }
    if (both || !std::strcmp(argv[1], "threads")) threads();
    std::printf("index_test: ok (%s)\n", both ? "exact, threads" : argv[1]);
    return 0;
}
