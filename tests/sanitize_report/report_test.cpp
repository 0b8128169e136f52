// report_test.cpp — the RX batch report's rules and host form (report_core.hpp, report.cpp) under
// ASan + UBSan: a stand-alone program, no HIP.
//   directed  every status x every header type, subtype and version x the lengths around the header
//             and the tag x with and without a tunnel, own-source marks, padding slots and entry
//             indexes past from[], in all three source modes and relayed;
//   random    random batches;
//   hostile   lengths and offsets past the arena (refused, nothing written), entry indexes past nfrom.
// Every input sits in a heap buffer of exactly its length, the arena ends with the last packet's
// last byte, and every output has exactly n records, so a read or write past an end is caught. The
// results are compared with the per-packet walk restated here.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "../../include/nebula_aead.h"
#include "../../nebula_amd/csrc/report_core.hpp"

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::abort();                                             \
        }                                                             \
    } while (0)

namespace {

template <class T>
struct Exact {  // a heap buffer of exactly n elements (n == 0: a null pointer)
    T* p;
    size_t n;
    explicit Exact(size_t n_) : p(n_ ? (T*)std::malloc(n_ * sizeof(T)) : nullptr), n(n_) {
        CHECK(!n_ || p);
        if (n) std::memset(p, 0xA5, n * sizeof(T));
    }
    explicit Exact(const std::vector<T>& v) : Exact(v.size()) {
        if (n) std::memcpy(p, v.data(), n * sizeof(T));
    }
    ~Exact() { std::free(p); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

struct Pkt {
    int32_t status;
    uint32_t type, sub, ver, len, key, index, entry;  // entry: into from[], as given
    bool own;
};
enum Mode { kEntry, kPacket, kNone };
struct Batch {
    std::vector<Pkt> p;
    std::vector<neb_udp_addr> from;  // kEntry: the entries; kPacket: rebuilt per packet from them
    Mode mode = kEntry;
    bool relayed = false;
};

neb_udp_addr addr(uint8_t last, uint16_t port, uint8_t family) {
    neb_udp_addr a{};
    a.addr[0] = 10, a.addr[family == 4 ? 3 : 15] = last, a.port = port, a.family = family;
    return a;
}

// The arrays the call takes. Packets lie back to back in arrival order, the last one ends the arena.
struct Arrays {
    std::vector<neb_rx_packet> pk;
    std::vector<int32_t> status;
    std::vector<uint8_t> arena;
    std::vector<neb_udp_addr> from;
    std::vector<uint32_t> entry;
};
Arrays lay_out(const Batch& b) {
    Arrays a;
    for (const Pkt& p : b.p) {
        const uint64_t off = a.arena.size();
        a.pk.push_back({off, p.len | (p.own ? NEB_RX_OWN_SOURCE : 0u), p.key});
        a.status.push_back(p.status);
        uint8_t h[16] = {(uint8_t)(p.ver << 4 | p.type), (uint8_t)p.sub, 0, 0, (uint8_t)(p.index >> 24), (uint8_t)(p.index >> 16),
                         (uint8_t)(p.index >> 8), (uint8_t)p.index};
        for (uint32_t k = 0; k < p.len; k++) a.arena.push_back(k < 16 ? h[k] : 0xEE);
        if (b.mode == kEntry) a.entry.push_back(p.entry);
        if (b.mode == kPacket) a.from.push_back(p.entry < b.from.size() ? b.from[p.entry] : neb_udp_addr{});
    }
    if (b.mode == kEntry) a.from = b.from;
    return a;
}

struct Run {
    uint64_t bytes;
    uint32_t key, packet, packets;
    neb_udp_addr from;
};
struct Want {
    std::vector<Run> runs;
    std::vector<std::pair<uint32_t, uint32_t>> used, work;
    uint64_t m[16] = {};
    uint32_t ntunnels = 0;
};
bool valid_sub(uint32_t t, uint32_t s) { return (t == 1 || t == 4) ? s <= 1 : (t == 0 || (t >= 2 && t <= 6)) && s == 0; }

// readOutsidePackets' bookkeeping packet by packet, with the finished status in place of the lookups
// and the decrypt.
Want walk(const Batch& b) {
    Want w;
    std::map<uint32_t, std::vector<uint32_t>> tunnels;  // key -> its authenticated packets, in order
    std::map<uint32_t, uint32_t> used;
    auto source = [&](uint32_t i) {
        const uint32_t e = b.p[i].entry;
        return b.mode == kNone || b.relayed || e == NEB_RECV_NONE || e >= b.from.size() ? neb_udp_addr{} : b.from[e];
    };
    for (uint32_t i = 0; i < b.p.size(); i++) {
        const Pkt& p = b.p[i];
        const bool has = p.len >= 16, no_tunnel = p.status == NEB_STATUS_BAD_KEY && p.key == NEB_KEYS_MIXED;
        if (p.status == NEB_STATUS_INVALID && p.len > 1) w.m[NEB_METRIC_RX_INVALID]++;
        if (has && p.ver == 1 && valid_sub(p.type, p.sub) && (b.relayed || !p.own) && p.type != 1) {
            const uint32_t slot[7] = {0, 0, 1, 2, p.sub ? 4u : 3u, 5, 6};
            w.m[slot[p.type]]++;
        }
        uint32_t kind = 0;
        if (p.status == NEB_STATUS_NOT_MESSAGE && has)
            kind = p.type == 0 ? 1 : p.type == 2 ? 2 : (b.relayed && p.type == 1 && p.sub == 1) ? 3 : 0;
        else if (no_tunnel) {
            w.m[NEB_METRIC_NO_TUNNEL]++;
            kind = has && !b.relayed ? 4 : 0;
        } else if (p.status == NEB_STATUS_AUTH_FAILED)
            w.m[NEB_METRIC_AUTH_FAILED]++;
        else if (p.status == NEB_STATUS_REPLAY)
            w.m[NEB_METRIC_REPLAY]++;
        else if (p.status == NEB_STATUS_OK) {
            w.m[NEB_METRIC_OPENED]++;
            w.m[NEB_METRIC_OPENED_BYTES] += p.len;
            tunnels[p.key].push_back(i);
            if (has && p.type == 1 && p.sub == 1) used[p.index]++;
            if (has) kind = p.type == 3 ? 5 : (p.type == 4 && p.sub == 0) ? 6 : p.type == 5 ? 7 : p.type == 6 ? 8 : 0;
        }
        if (kind) w.work.push_back({i, kind});
    }
    for (const auto& t : tunnels) {
        for (uint32_t i : t.second) {
            const neb_udp_addr f = source(i);
            if (i == t.second[0] || std::memcmp(&f, &w.runs.back().from, sizeof f))
                w.runs.push_back({0, t.first, i, 0, f});
            w.runs.back().bytes += b.p[i].len;
            w.runs.back().packets++;
        }
    }
    w.ntunnels = (uint32_t)tunnels.size();
    w.used.assign(used.begin(), used.end());
    return w;
}

int call(const Arrays& a, const Batch& b, Exact<uint8_t>& arena, Exact<neb_rx_run>& runs, Exact<neb_rx_relay_used>& used,
         Exact<neb_rx_work>& work, uint64_t* m, uint32_t* c) {
    Exact<neb_rx_packet> pk(a.pk);
    Exact<int32_t> st(a.status);
    Exact<neb_udp_addr> from(a.from);
    Exact<uint32_t> entry(a.entry);
    return neb_rx_report_batch_host(pk.p, st.p, (uint32_t)a.pk.size(), arena.p, arena.n, b.mode == kNone ? nullptr : from.p,
                                    b.mode == kEntry ? entry.p : nullptr, (uint32_t)from.n, b.relayed ? NEB_REPORT_RELAYED : 0u,
                                    runs.p, used.p, work.p, m, c);
}

void check(const Batch& b) {
    const Arrays a = lay_out(b);
    const size_t n = a.pk.size();
    Exact<uint8_t> arena(a.arena.empty() ? std::vector<uint8_t>{0} : a.arena);
    if (a.arena.empty()) arena.n = 0;  // a valid pointer to nothing
    Exact<neb_rx_run> runs(n);
    Exact<neb_rx_relay_used> used(n);
    Exact<neb_rx_work> work(n);
    Exact<uint64_t> m(16);
    Exact<uint32_t> c(4);
    CHECK(call(a, b, arena, runs, used, work, m.p, c.p) == NEB_OK);
    const Want w = walk(b);
    CHECK(c.p[0] == w.runs.size() && c.p[1] == w.ntunnels && c.p[2] == w.used.size() && c.p[3] == w.work.size());
    CHECK(!std::memcmp(m.p, w.m, sizeof w.m));
    for (size_t r = 0; r < w.runs.size(); r++) {
        const neb_rx_run& g = runs.p[r];
        const Run& e = w.runs[r];
        CHECK(g.bytes == e.bytes && g.key_id == e.key && g.packet == e.packet && g.packets == e.packets &&
              !std::memcmp(&g.from, &e.from, sizeof e.from));
    }
    for (size_t r = 0; r < w.used.size(); r++) CHECK(used.p[r].index == w.used[r].first && used.p[r].packets == w.used[r].second);
    for (size_t r = 0; r < w.work.size(); r++) CHECK(work.p[r].packet == w.work[r].first && work.p[r].kind == w.work[r].second);
    const uint8_t* tail = (const uint8_t*)(runs.p + w.runs.size());
    for (size_t k = 0; k < (n - w.runs.size()) * sizeof(neb_rx_run); k++) CHECK(tail[k] == 0xA5);  // nothing past the count
}

const std::vector<neb_udp_addr> kFrom = {addr(1, 4242, 4), addr(2, 4242, 4), addr(1, 4243, 4), addr(1, 4242, 6)};

void directed() {
    for (int relayed = 0; relayed < 2; relayed++)
        for (Mode mode : {kEntry, kPacket, kNone}) {
            Batch b;
            b.mode = mode, b.relayed = relayed, b.from = kFrom;
            uint32_t k = 0;
            for (int32_t st = -1; st < 18; st++)
                for (uint32_t t = 0; t < 8; t++)
                    for (uint32_t s = 0; s < 3; s++)
                        for (uint32_t len : {0u, 1u, 2u, 15u, 16u, 31u, 32u, 48u}) {
                            const uint32_t entries[6] = {0, 1, 2, 3, NEB_RECV_NONE, 4 + k};  // the last two: no source
                            b.p.push_back({st, t, s, k % 11 ? 1u : 2u, len, k % 3 ? 7u + (k % 2 << 31) : NEB_KEYS_MIXED,
                                           0x80000000u >> (k % 4), entries[k % 6], k % 13 == 0});
                            k++;
                        }
            check(b);
        }
    check(Batch{});  // n == 0
}

void random_batches() {
    std::mt19937 gen(20261);
    auto rng = [&]() { return (uint32_t)gen(); };
    for (int round = 0; round < 300; round++) {
        Batch b;
        b.mode = Mode(round % 3), b.relayed = round % 4 == 3, b.from = kFrom;
        const uint32_t n = 1 + rng() % (round % 10 ? 40 : 3000), ntun = 1 + rng() % 40;
        const int32_t sts[8] = {0, 0, 0, 0, 1, 3, 4, 5};
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t lens[6] = {0, 16, 32, 64, 200, 1364};
            b.p.push_back({rng() % 5 ? sts[rng() % 8] : (int32_t)(rng() % 19) - 1, rng() % 4 ? 1u : rng() % 8, rng() % 3, 1, lens[rng() % 6],
                           rng() % 20 ? rng() % ntun : NEB_KEYS_MIXED, rng() % 4, rng() % 10 ? rng() % 4 : rng(), rng() % 30 == 0});
        }
        check(b);
    }
}

void hostile() {
    Batch b;
    b.from = kFrom;
    for (uint32_t i = 0; i < 6; i++) b.p.push_back({0, 1, 0, 1, 64, 7, 1, 0, false});
    Arrays a = lay_out(b);
    Exact<uint8_t> arena(a.arena);
    Exact<neb_rx_run> runs(6);
    Exact<neb_rx_relay_used> used(6);
    Exact<neb_rx_work> work(6);
    uint64_t m[16];
    uint32_t c[4];
    auto refused = [&]() {
        std::memset(m, 0xA5, sizeof m), std::memset(c, 0xA5, sizeof c);
        CHECK(call(a, b, arena, runs, used, work, m, c) == NEB_ERR_INVALID);
        CHECK(m[0] == 0xA5A5A5A5A5A5A5A5ull && c[0] == 0xA5A5A5A5u && ((const uint8_t*)runs.p)[0] == 0xA5);
    };
    CHECK(call(a, b, arena, runs, used, work, m, c) == NEB_OK && c[0] == 1);
    std::memset(runs.p, 0xA5, sizeof(neb_rx_run));
    const uint64_t end = a.arena.size();
    const std::pair<uint32_t, neb_rx_packet> bad[] = {
        {5, {a.pk[5].off, 65, 7}},  // one byte past the arena
        {5, {a.pk[5].off + 1, 64 | NEB_RX_OWN_SOURCE, 7}},
        {3, {end - 15, 16, 7}},
        {3, {end + 1, 16, 7}},
        {0, {~0ull, 16, 7}},
        {0, {~0ull - 14, 16, 7}},
        {2, {1ull << 63, 0x7FFFFFFFu, 7}},
        {2, {0, 0x7FFFFFFFu | NEB_RX_OWN_SOURCE, 7}},
    };
    for (const auto& [i, p] : bad) {
        const neb_rx_packet good = a.pk[i];
        a.pk[i] = p;
        refused();
        a.pk[i] = good;
    }
    const neb_rx_packet good = a.pk[3];
    a.pk[3] = neb_rx_packet{~0ull, 15, 7};  // no header: its offset is never used
    CHECK(call(a, b, arena, runs, used, work, m, c) == NEB_OK && m[NEB_METRIC_OPENED] == 6);
    a.pk[3] = good;
    // entry indexes past from[]: never read (from[] is exactly four records)
    for (uint32_t e : {4u, 5u, 0x7FFFFFFFu, 0xFFFFFFFEu, NEB_RECV_NONE}) {
        a.entry[2] = e;
        CHECK(call(a, b, arena, runs, used, work, m, c) == NEB_OK && c[0] == 3 && runs.p[1].from.family == 0);
    }
}

}  // namespace

int main() {
    directed();
    random_batches();
    hostile();
    std::printf("report_test: ok (directed, random, hostile)\n");
    return 0;
}
