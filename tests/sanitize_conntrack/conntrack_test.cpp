// conntrack_test.cpp — the connection table's rules, host-only table and host forms
// (conntrack_core.hpp, conntrack.cpp) under sanitizers: a stand-alone program, no HIP.
//   (no argument)  exact: random batches of lookups, adds and evicts, with compactions, against a
//                  linear-scan model, every array a heap buffer of exactly its length (so nothing
//                  past a batch's last record is read or written), at capacities 1, 4 and 257; the
//                  threads once; and two copies of a new key interleaved at the table's last place.
//   threads        one adding and evicting thread against two looking-up ones: a steady key never
//                  misses, and a key removed before a lookup began never hits in it.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nebula_aead.h"
#include "../../nebula_amd/csrc/conntrack_core.hpp"

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::abort();                                                \
        }                                                                \
    } while (0)

namespace {

constexpr uint64_t kTcp = 7000, kUdp = 300, kDefault = 50;

neb_fw_packet key(uint32_t i) {
    neb_fw_packet p{};
    p.family = i % 3 == 2 ? 6 : 4;
    p.local_addr[0] = 10, p.local_addr[3] = (uint8_t)i;
    p.remote_addr[0] = 10, p.remote_addr[2] = (uint8_t)(i >> 8), p.remote_addr[3] = 9;
    if (p.family == 6) p.remote_addr[15] = (uint8_t)(i >> 4);
    else std::memset(p.local_addr + 4, 0xA5, 12);  // not part of a v4 key
    p.local_port = (uint16_t)(1000 + i % 7), p.remote_port = (uint16_t)(i * 31);
    p.protocol = i % 4 == 0 ? 6 : i % 4 == 1 ? 17 : 1;
    p.flags = (uint8_t)((i % 5 == 0 ? NEB_FW_FRAGMENT : 0) | NEB_FW_ROUTED);
    p.gateway = i;
    return p;
}

// An exact-size heap copy: ASan sees the first byte past it.
template <class T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

struct Conn {
    neb::CtKey k;
    uint64_t expires;
    uint32_t incoming, version;
};
struct Model {
    uint32_t capacity, version = 0;
    std::vector<Conn> conns;
    int find(const neb::CtKey& k) const {
        for (size_t i = 0; i < conns.size(); i++)
            if (neb::ct_key_eq(conns[i].k, k)) return (int)i;
        return -1;
    }
    static uint64_t timeout(const neb::CtKey& k) {
        const uint32_t p = neb::ct_key_protocol(k);
        return p == 6 ? kTcp : p == 17 ? kUdp : kDefault;
    }
};

void check_image(neb_conntrack* t, const Model& m) {
    uint64_t c[3];
    CHECK(neb_conntrack_count(t, c) == NEB_OK && c[0] == m.conns.size());
    std::vector<neb::CtSlot> img(c[2]);
    CHECK(neb_conntrack_dump(t, img.data(), (uint32_t)c[2]) == NEB_OK);
    size_t settled = 0, tombs = 0;
    for (const neb::CtSlot& s : img) {
        tombs += s.state == neb::kCtTomb;
        if ((s.state & neb::kCtKindMask) != neb::kCtSettled) {
            CHECK(s.state == neb::kCtEmpty || s.state == neb::kCtTomb);
            continue;
        }
        settled++;
        neb::CtKey k;
        std::memcpy(k.w, s.key, sizeof k.w);
        const int at = m.find(k);
        CHECK(at >= 0 && m.conns[at].expires == s.expires && s.meta == neb::ct_meta(m.conns[at].version, m.conns[at].incoming));
    }
    CHECK(settled == m.conns.size() && tombs == c[1]);
}

void random_script(uint32_t capacity, uint32_t universe, uint32_t seed) {
    std::mt19937 rng(seed);
    neb_conntrack* t = nullptr;
    CHECK(neb_conntrack_create(nullptr, capacity, 0xC0FFEEull + seed, kTcp, kUdp, kDefault, 300, &t) == NEB_OK);
    Model m{capacity};
    uint64_t now = 1000000;
    const uint32_t sizes[] = {1, 2, 63, 64, 65, 255, 256, 257};
    for (int step = 0; step < 400; step++) {
        const uint32_t n = sizes[rng() % 8];
        std::vector<neb_fw_packet> fw(n);
        for (auto& p : fw) p = key(rng() % universe);
        const auto d_fw = exact(fw);
        now += rng() % 200;
        const uint32_t op = rng() % 10;
        if (op < 4) {  // lookup
            std::vector<int32_t> st(n);
            for (auto& s : st) s = rng() % 8 ? NEB_STATUS_OK : NEB_STATUS_REPLAY;
            const bool hold = rng() % 2;
            const uint32_t cap = rng() % 3 == 0 ? 0 : rng() % 3 == 1 ? n / 2 : n;
            std::vector<neb_plain_packet> plain(n);
            std::vector<neb_tx_packet> tx(n);
            for (uint32_t i = 0; i < n; i++) plain[i].flags = NEB_PLAIN_PARSED, tx[i].tunnel = i;
            const auto d_st = exact(st);
            const auto d_plain = exact(plain);
            const auto d_tx = exact(tx);
            std::unique_ptr<uint8_t[]> verdict(new uint8_t[n]);
            std::unique_ptr<neb_ct_work[]> work(new neb_ct_work[cap]);
            std::unique_ptr<uint32_t[]> counts(new uint32_t[4]);
            CHECK(neb_conntrack_lookup_batch_host(t, d_fw.get(), d_st.get(), n, now, verdict.get(), hold ? d_plain.get() : nullptr,
                                                  hold ? d_tx.get() : nullptr, cap ? work.get() : nullptr, cap,
                                                  counts.get()) == NEB_OK);
            uint32_t want[4] = {0, 0, 0, 0};
            for (uint32_t i = 0; i < n; i++) {
                uint32_t v = NEB_CT_NONE;
                if (st[i] == NEB_STATUS_OK) {
                    const neb::CtKey k = neb::ct_key_of(&fw[i]);
                    const int at = m.find(k);
                    if (at < 0) v = NEB_CT_MISS;
                    else if (m.conns[at].version != m.version) v = NEB_CT_STALE | (m.conns[at].incoming ? NEB_CT_INCOMING : 0);
                    else {
                        v = NEB_CT_HIT;
                        if (now + Model::timeout(k) > m.conns[at].expires) m.conns[at].expires = now + Model::timeout(k);
                    }
                    want[(v & 0x7F) - 1]++;
                }
                CHECK(verdict[i] == v);
                const bool held = hold && v != NEB_CT_NONE && v != NEB_CT_HIT;
                CHECK(d_st[i] == (held ? NEB_STATUS_FW_HELD : st[i]));
                CHECK(d_plain[i].flags == (NEB_PLAIN_PARSED | (held ? NEB_PLAIN_SKIP : 0)));
                CHECK(d_tx[i].tunnel == (held ? NEB_TX_NO_TUNNEL : i));
                if (v > NEB_CT_HIT) {
                    if (want[3] < cap) {
                        const neb_ct_work& w = work[want[3]];
                        CHECK(w.packet == i && w.verdict == v && !std::memcmp(&w.fw, &fw[i], sizeof w.fw));
                    }
                    want[3]++;
                }
            }
            CHECK(!std::memcmp(want, counts.get(), sizeof want));
        } else if (op < 7) {  // add
            uint64_t c[3];
            CHECK(neb_conntrack_count(t, c) == NEB_OK);
            if (c[1] >= c[2] - capacity) CHECK(neb_conntrack_compact(t, nullptr) == NEB_OK);  // an EMPTY slot for every new key
            std::vector<uint8_t> inc(n);
            for (auto& b : inc) b = (uint8_t)(rng() % 2);
            const auto d_inc = exact(inc);
            std::unique_ptr<neb_ct_result[]> res(new neb_ct_result[n]);
            CHECK(neb_conntrack_add_batch_host(t, d_fw.get(), d_inc.get(), n, now, res.get()) == NEB_OK);
            std::vector<neb::CtKey> seen;
            for (uint32_t i = 0; i < n; i++) {
                const neb::CtKey k = neb::ct_key_of(&fw[i]);
                bool dup = false;
                for (const auto& s : seen) dup |= neb::ct_key_eq(s, k);
                const int at = m.find(k);
                uint32_t code;
                if (dup) {
                    code = NEB_CT_DUP;
                    m.conns[at].incoming = inc[i];
                } else if (at >= 0) {
                    code = NEB_CT_EXISTING;
                    m.conns[at] = Conn{k, now + Model::timeout(k), inc[i], m.version};
                    seen.push_back(k);
                } else if (m.conns.size() >= capacity) {
                    code = NEB_CT_FULL;
                } else {
                    code = NEB_CT_NEW;
                    m.conns.push_back(Conn{k, now + Model::timeout(k), inc[i], m.version});
                    seen.push_back(k);
                }
                CHECK(res[i].code == code && (res[i].slot == NEB_CT_NO_SLOT) == (code == NEB_CT_FULL));
            }
        } else if (op < 9) {  // evict
            const bool force = rng() % 3 == 0;
            std::unique_ptr<int64_t[]> rem(new int64_t[n]);
            CHECK(neb_conntrack_evict_batch_host(t, d_fw.get(), n, now, force, rem.get()) == NEB_OK);
            for (uint32_t i = 0; i < n; i++) {
                const int at = m.find(neb::ct_key_of(&fw[i]));
                int64_t want = -1;
                if (at >= 0 && !force && m.conns[at].expires > now) want = (int64_t)(m.conns[at].expires - now);
                else if (at >= 0) {
                    want = 0;
                    m.conns.erase(m.conns.begin() + at);
                }
                CHECK(rem[i] == want);
            }
        } else {
            m.version = rng() % 3 == 0 ? 65535 : rng() % 3;
            CHECK(neb_conntrack_set_rules_version(t, (uint16_t)m.version) == NEB_OK);
        }
        check_image(t, m);
    }
    CHECK(neb_conntrack_compact(t, nullptr) == NEB_OK);
    check_image(t, m);
    CHECK(neb_conntrack_destroy(t) == NEB_OK);
}

// A copy of a new key finds its slot EMPTY; before it reads the live count, another copy claims the
// slot and takes the table's last place. The late copy must follow it (DUP, its incoming stored), not
// answer FULL beside a NEW. The policy runs the other copy's whole claim inside the load of the count.
struct InterleaveMem : neb::CtHostMem {
    const uint64_t* live;
    std::function<void()>* inside;
    uint64_t load(const uint64_t* p) const {
        if (p == live && *inside) {
            const std::function<void()> f = std::move(*inside);
            *inside = nullptr;
            f();
        }
        return neb::CtHostMem::load(p);
    }
};

void interleaved_copies() {
    const neb::CtParams p{7, kTcp, kUdp, kDefault, 1, 1};  // capacity 1, two slots
    std::vector<neb::CtSlot> slots(2);
    uint64_t counters[2] = {0, 0};
    const neb_fw_packet fw = key(3);
    const neb::CtKey k = neb::ct_key_of(&fw);
    auto key_of = [&](uint32_t) { return k; };
    neb::CtAdd r[2];
    std::function<void()> inside = [&] {
        r[0] = neb::ct_add_claim(slots.data(), &counters[0], p, 0, 100, 0, k, 0, key_of, neb::CtHostMem{});
    };
    InterleaveMem m;
    m.live = &counters[0], m.inside = &inside;
    r[1] = neb::ct_add_claim(slots.data(), &counters[0], p, 0, 100, 1, k, 1, key_of, m);
    CHECK(!inside && r[0].code == NEB_CT_NEW && r[1].code == NEB_CT_DUP && r[0].slot == r[1].slot);
    auto code_of = [&](uint32_t j) { return r[j].code; };
    for (auto& x : r) x = neb::ct_add_settle(slots.data(), counters, x, code_of, neb::CtHostMem{});
    CHECK(r[0].code == NEB_CT_NEW && r[1].code == NEB_CT_DUP && counters[0] == 1 && counters[1] == 0);
    CHECK(slots[r[0].slot].meta == neb::ct_meta(0, 1));  // the highest index's incoming
    // and the other way round: the table full before either copy claims -> both FULL, nothing changed
    std::vector<neb::CtSlot> full(2);
    uint64_t c2[2] = {1, 0};
    for (uint32_t i = 0; i < 2; i++) r[i] = neb::ct_add_claim(full.data(), &c2[0], p, 0, 100, i, k, i, key_of, neb::CtHostMem{});
    CHECK(r[0].code == NEB_CT_FULL && r[1].code == NEB_CT_FULL && c2[0] == 1 && full[0].state == 0 && full[1].state == 0);
}

void threads() {
    constexpr uint32_t kSteady = 64, kChurn = 256, kRounds = 300;
    neb_conntrack* t = nullptr;
    CHECK(neb_conntrack_create(nullptr, 512, 42, kTcp, kUdp, kDefault, 512, &t) == NEB_OK);
    std::vector<neb_fw_packet> steady(kSteady), churn(kChurn);
    for (uint32_t i = 0; i < kSteady; i++) steady[i] = key(i);
    for (uint32_t i = 0; i < kChurn; i++) churn[i] = key(1000 + i);
    std::vector<uint8_t> inc(kChurn, 1);
    std::vector<neb_ct_result> res(kChurn);
    CHECK(neb_conntrack_add_batch_host(t, steady.data(), inc.data(), kSteady, 1, res.data()) == NEB_OK);
    // phase: odd while the churn keys may be in the table, even (and 2 more each round) once they are gone
    std::atomic<uint32_t> phase{0};
    std::atomic<bool> stop{false};
    auto looker = [&](uint32_t id) {
        std::vector<int32_t> st(kChurn, NEB_STATUS_OK);
        std::vector<uint8_t> v(kChurn);
        uint32_t counts[4];
        uint64_t now = 10 + id;
        while (!stop.load(std::memory_order_acquire)) {
            CHECK(neb_conntrack_lookup_batch_host(t, steady.data(), st.data(), kSteady, now++, v.data(), nullptr, nullptr, nullptr, 0,
                                                  counts) == NEB_OK);
            CHECK(counts[0] == kSteady && counts[3] == 0);  // a steady key never misses
            const uint32_t before = phase.load(std::memory_order_acquire);
            CHECK(neb_conntrack_lookup_batch_host(t, churn.data(), st.data(), kChurn, now++, v.data(), nullptr, nullptr, nullptr, 0,
                                                  counts) == NEB_OK);
            const uint32_t after = phase.load(std::memory_order_acquire);
            // removed before the lookup began and not added again before it ended: no hit
            if (before == after && before % 2 == 0) CHECK(counts[0] == 0 && counts[1] == kChurn);
        }
    };
    std::thread a(looker, 0), b(looker, 1);
    std::vector<int64_t> rem(kChurn);
    for (uint32_t r = 0; r < kRounds; r++) {
        phase.fetch_add(1, std::memory_order_acq_rel);
        CHECK(neb_conntrack_add_batch_host(t, churn.data(), inc.data(), kChurn, 100 + r, res.data()) == NEB_OK);
        for (const auto& x : res) CHECK(x.code == NEB_CT_NEW);
        CHECK(neb_conntrack_evict_batch_host(t, churn.data(), kChurn, 100 + r, 1, rem.data()) == NEB_OK);
        for (int64_t x : rem) CHECK(x == 0);
        phase.fetch_add(1, std::memory_order_acq_rel);
        uint64_t c[3];
        CHECK(neb_conntrack_count(t, c) == NEB_OK && c[0] == kSteady);
        if (c[1] + kChurn + kSteady >= c[2]) {  // tombstones: nothing may run during a compaction
            stop.store(true, std::memory_order_release);
            a.join(), b.join();
            CHECK(neb_conntrack_compact(t, nullptr) == NEB_OK);
            stop.store(false, std::memory_order_release);
            a = std::thread(looker, 0), b = std::thread(looker, 1);
        }
    }
    stop.store(true, std::memory_order_release);
    a.join(), b.join();
    CHECK(neb_conntrack_destroy(t) == NEB_OK);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "threads") {
        threads();
        std::printf("conntrack_test: ok (threads)\n");
        return 0;
    }
    interleaved_copies();
    random_script(1, 4, 1);
    random_script(4, 7, 2);
    random_script(257, 400, 3);
    threads();
    std::printf("conntrack_test: ok (exact, threads)\n");
    return 0;
}
