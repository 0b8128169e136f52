// route_test.cpp — the TX table's rules, host table and host form (route_core.hpp, route.cpp) under
// sanitizers: a stand-alone program, no HIP.
//   (no argument)  exact: every truncation of a set of packet templates resolved from a heap buffer
//                  of exactly its length; random host updates (enough of them between two route
//                  replacements for the table to rebuild itself, which the program checks) and
//                  route replacements against a linear-scan model, the batch in an arena that ends
//                  with its last packet; then the threads once.
//   threads        two updating threads against two resolving ones: a steady address never misses,
//                  and every batch equals the old or the new route set as a whole.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nebula_aead.h"

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::abort();                                             \
        }                                                             \
    } while (0)

namespace {

neb_tx_addr addr4(uint32_t a) {
    neb_tx_addr r{};
    r.family = 4;
    for (int i = 0; i < 4; i++) r.addr[i] = (uint8_t)(a >> (24 - 8 * i));
    return r;
}
neb_cidr cidr4(uint32_t a, uint32_t bits) {
    neb_cidr c{};
    c.family = 4;
    c.bits = (uint8_t)bits;
    for (int i = 0; i < 4; i++) c.addr[i] = (uint8_t)(a >> (24 - 8 * i));
    return c;
}
neb_route route4(uint32_t a, uint32_t bits, std::vector<std::pair<uint32_t, uint32_t>> gws) {
    neb_route r{};
    r.prefix = cidr4(a, bits);
    r.ngateways = (uint32_t)gws.size();
    for (size_t k = 0; k < gws.size(); k++) {
        r.gateways[k].addr = addr4(gws[k].first);
        r.gateways[k].weight = gws[k].second;
    }
    return r;
}
std::vector<uint8_t> udp4(uint32_t dst, uint16_t sport, uint16_t dport) {
    std::vector<uint8_t> p(32, 0);
    p[0] = 0x45;
    p[3] = 32;
    p[9] = 17;
    p[12] = 10, p[13] = 1, p[14] = 0, p[15] = 7;
    for (int i = 0; i < 4; i++) p[16 + i] = (uint8_t)(dst >> (24 - 8 * i));
    p[20] = (uint8_t)(sport >> 8), p[21] = (uint8_t)sport, p[22] = (uint8_t)(dport >> 8), p[23] = (uint8_t)dport;
    return p;
}

// One packet from a heap buffer of exactly its length.
void resolve_exact(neb_tx_table* t, const std::vector<uint8_t>& p, uint32_t* tunnel, int32_t* status, neb_fw_packet* fw) {
    uint8_t* buf = p.empty() ? nullptr : (uint8_t*)std::malloc(p.size());
    if (!p.empty()) std::memcpy(buf, p.data(), p.size());
    neb_tx_packet pk{};
    pk.len = (uint32_t)p.size();
    CHECK(neb_tx_resolve_batch_host(t, &pk, 1, buf, p.size(), fw, status) == NEB_OK);
    *tunnel = pk.tunnel;
    std::free(buf);
}

constexpr uint32_t kNet = 0x0A010000u;  // 10.1.0.0/24, own address .7
void set_own(neb_tx_table* t) {
    neb_cidr own = cidr4(kNet | 7u, 24);
    CHECK(neb_tx_table_set_own(t, &own, 1, NEB_TX_DROP_LOCAL_BROADCAST | NEB_TX_DROP_MULTICAST) == NEB_OK);
}

void truncations(neb_tx_table* t) {
    std::vector<std::vector<uint8_t>> tpl;
    tpl.push_back(udp4(kNet | 20u, 1, 2));
    {  // IHL 24, ICMP
        std::vector<uint8_t> p = udp4(kNet | 20u, 1, 2);
        p[0] = 0x46;
        p[9] = 1;
        p.resize(40, 0);
        tpl.push_back(p);
    }
    {  // IPv6: hop-by-hop, routing, fragment (first), AH, destination options, then ICMPv6 echo
        std::vector<uint8_t> p(40, 0);
        p[0] = 0x60;
        p[6] = 0;
        p[8] = 0xfd, p[24] = 0xfd, p[39] = 9;
        const uint8_t next[] = {43, 44, 51, 60, 58};
        for (int k = 0; k < 5; k++) {
            std::vector<uint8_t> e(next[k] == 60 /* this one is the AH */ ? 12 : 8, 0);
            e[0] = next[k];
            if (e.size() == 12) e[1] = 1;
            p.insert(p.end(), e.begin(), e.end());
        }
        const uint8_t echo[8] = {128, 0, 0, 0, 0x12, 0x34, 0, 1};
        p.insert(p.end(), echo, echo + 8);
        tpl.push_back(p);
        std::vector<uint8_t> q = p;  // a non-first fragment, and an extension length past the end
        q[40 + 8 + 8 + 2] = 1;
        tpl.push_back(q);
        q = p;
        q[41] = 255;
        tpl.push_back(q);
    }
    for (const auto& p : tpl)
        for (size_t cut = 0; cut <= p.size(); cut++) {
            uint32_t tunnel;
            int32_t status;
            neb_fw_packet fw;
            resolve_exact(t, std::vector<uint8_t>(p.begin(), p.begin() + cut), &tunnel, &status, &fw);
            CHECK(status == NEB_STATUS_INVALID || status == NEB_STATUS_OK || status == NEB_STATUS_NO_TUNNEL ||
                  status == NEB_STATUS_NO_ROUTE);
            CHECK((status == NEB_STATUS_OK) == (tunnel != NEB_TX_NO_TUNNEL));
        }
}

struct Model {
    std::map<uint32_t, uint32_t> hosts;
    struct R {
        uint32_t addr, bits;
        std::vector<std::pair<uint32_t, uint32_t>> gws;
    };
    std::vector<R> routes;
    void expect(uint32_t dst, uint32_t* tunnel, int32_t* status) const {
        *tunnel = NEB_TX_NO_TUNNEL;
        if ((dst & 0xFFFFFF00u) == kNet) {
            if (dst == (kNet | 255u) || dst == (kNet | 7u)) { *status = NEB_STATUS_TX_DROPPED; return; }
            auto it = hosts.find(dst);
            *status = it == hosts.end() ? NEB_STATUS_NO_TUNNEL : NEB_STATUS_OK;
            if (it != hosts.end()) *tunnel = it->second;
            return;
        }
        const R* best = nullptr;
        for (const R& r : routes) {
            const uint32_t m = r.bits ? ~0u << (32 - r.bits) : 0u;
            if ((dst & m) == (r.addr & m) && (!best || r.bits > best->bits)) best = &r;
        }
        if (!best) { *status = NEB_STATUS_NO_ROUTE; return; }
        auto it = hosts.find(best->gws[0].first);  // the model's routes have one gateway
        *status = it == hosts.end() ? NEB_STATUS_NO_TUNNEL : NEB_STATUS_OK;
        if (it != hosts.end()) *tunnel = it->second;
    }
};

void random_updates(neb_tx_table* t) {
    std::mt19937 rng(11);
    Model m;
    // 28 addresses keep the table under its capacity of 32, so the puts go through and fill the
    // slots until a host update rebuilds the table; a burst over a wider range must be refused whole
    auto pool = [&] { return kNet | (20u + rng() % 28u); };
    const uint32_t hot = kNet | 20u;
    const neb_cidr hot_key = cidr4(hot, 32);
    uint32_t last_probes = 0, rebuilds = 0;
    for (int step = 0; step < 600; step++) {
        std::vector<neb_tx_addr> del;
        std::vector<neb_tx_host> put;
        Model next = m;
        if (step % 97 == 96)
            for (uint32_t k = 0; k < 40; k++) {
                put.push_back(neb_tx_host{addr4(kNet | (120u + k)), k});
                next.hosts[kNet | (120u + k)] = k;
            }
        for (uint32_t k = rng() % 4; k; k--) {
            const uint32_t a = pool();
            del.push_back(addr4(a));
            next.hosts.erase(a);
        }
        for (uint32_t k = rng() % 6; k; k--) {
            const uint32_t a = pool(), tun = rng() % 100;
            put.push_back(neb_tx_host{addr4(a), tun});
            next.hosts[a] = tun;
        }
        put.push_back(neb_tx_host{addr4(hot), (uint32_t)step});  // replaced every step: its chain grows
        next.hosts[hot] = (uint32_t)step;
        const int rc = neb_tx_table_update_hosts(t, del.data(), (uint32_t)del.size(), put.data(), (uint32_t)put.size(), nullptr);
        if (next.hosts.size() > 32) CHECK(rc == NEB_ERR_NO_KEY_SLOT);  // and nothing applied
        else {
            CHECK(rc == NEB_OK);
            m = next;
        }
        uint32_t probe[3];
        CHECK(neb_tx_table_probe(t, NEB_TX_KIND_HOST, &hot_key, probe) == NEB_OK && probe[0] == 1);
        if (rc == NEB_OK && probe[2] < last_probes) rebuilds++;  // a chain only shrinks in a rebuild
        if (step % 150 == 0) {
            std::vector<neb_route> routes;
            m.routes.clear();
            for (uint32_t k = rng() % 6; k; k--) {
                const uint32_t bits = 8 * (rng() % 4), addr = ((0x14000000u + (rng() % 3 << 16)) | (rng() % 2 << 8));
                const uint32_t mask = bits ? ~0u << (32 - bits) : 0u;
                bool dup = false;
                for (const auto& r : m.routes) dup |= r.bits == bits && (r.addr & mask) == (addr & mask);
                if (dup) continue;
                const uint32_t gw = pool();
                m.routes.push_back(Model::R{addr, bits, {{gw, 1}}});
                routes.push_back(route4(addr, bits, {{gw, 1}}));
            }
            CHECK(neb_tx_table_set_routes(t, routes.data(), (uint32_t)routes.size(), nullptr) == NEB_OK);
        }
        CHECK(neb_tx_table_probe(t, NEB_TX_KIND_HOST, &hot_key, probe) == NEB_OK);
        last_probes = probe[2];
        uint32_t hosts, nroutes;
        CHECK(neb_tx_table_count(t, &hosts, &nroutes) == NEB_OK && hosts == m.hosts.size() && nroutes == m.routes.size());
        // a batch in an arena that ends with its last packet, at odd offsets
        const uint32_t n = 24;
        std::vector<uint32_t> dst(n);
        std::vector<neb_tx_packet> pk(n);
        const size_t bytes = 1 + (size_t)n * 33 - 1;
        uint8_t* arena = (uint8_t*)std::malloc(bytes);
        std::memset(arena, 0xA5, bytes);
        for (uint32_t i = 0; i < n; i++) {
            dst[i] = i % 3 == 0 ? (0x14000000u | (rng() % 3 << 16) | (rng() % 2 << 8) | 9u) : i == 1 ? (kNet | 255u) : pool();
            const std::vector<uint8_t> p = udp4(dst[i], 5, 6);
            pk[i].in_off = 1 + (uint64_t)i * 33;
            pk[i].len = 32;
            std::memcpy(arena + pk[i].in_off, p.data(), 32);
        }
        std::vector<int32_t> status(n);
        std::vector<neb_fw_packet> fw(n);
        CHECK(neb_tx_resolve_batch_host(t, pk.data(), n, arena, bytes, fw.data(), status.data()) == NEB_OK);
        CHECK(neb_tx_resolve_batch_host(t, pk.data(), n, arena, bytes - 1, fw.data(), status.data()) == NEB_ERR_INVALID);
        for (uint32_t i = 0; i < n; i++) {
            uint32_t tunnel;
            int32_t st;
            m.expect(dst[i], &tunnel, &st);
            CHECK(status[i] == st && pk[i].tunnel == tunnel);
            CHECK(fw[i].local_port == 5 && fw[i].remote_port == 6 && fw[i].family == 4 && fw[i].ip_hdr_len == 20);
        }
        std::free(arena);
    }
    CHECK(rebuilds >= 3);  // the host updates alone rebuilt the table, and the model held across it
}

void threads() {
    neb_tx_table* t = nullptr;
    CHECK(neb_tx_table_create(nullptr, 32, 8, 8, &t) == NEB_OK);
    set_own(t);
    const uint32_t steady = kNet | 100u, gw_a = kNet | 101u, gw_b = kNet | 102u;
    const neb_tx_host base[3] = {{addr4(steady), 7}, {addr4(gw_a), 1}, {addr4(gw_b), 2}};
    CHECK(neb_tx_table_update_hosts(t, nullptr, 0, base, 3, nullptr) == NEB_OK);
    const std::vector<neb_route> set_a = {route4(0x14000000u, 8, {{gw_a, 1}}), route4(0x15000000u, 8, {{gw_a, 1}}), route4(0x15010000u, 16, {{gw_a, 1}})};
    const std::vector<neb_route> set_b = {route4(0x14000000u, 8, {{gw_b, 1}}), route4(0u, 0, {{gw_b, 1}})};
    CHECK(neb_tx_table_set_routes(t, set_a.data(), (uint32_t)set_a.size(), nullptr) == NEB_OK);
    std::atomic<bool> stop{false};
    std::vector<std::thread> th;
    th.emplace_back([&] {  // hosts come, go and are replaced; the steady address is replaced by itself
        std::mt19937 rng(1);
        for (int k = 0; k < 4000; k++) {
            const neb_tx_addr del = addr4(kNet | (110u + rng() % 20u));
            const neb_tx_host put[2] = {{addr4(kNet | (110u + rng() % 20u)), 50}, {addr4(steady), 7}};
            CHECK(neb_tx_table_update_hosts(t, &del, 1, put, 2, nullptr) == NEB_OK);
        }
        stop = true;
    });
    th.emplace_back([&] {
        for (int k = 0; !stop; k++) {
            const auto& s = k & 1 ? set_a : set_b;
            CHECK(neb_tx_table_set_routes(t, s.data(), (uint32_t)s.size(), nullptr) == NEB_OK);
        }
    });
    for (int r = 0; r < 2; r++)
        th.emplace_back([&] {
            const uint32_t dst[4] = {steady, 0x14010101u, 0x15010101u, 0x15020202u};
            std::vector<uint8_t> arena;
            neb_tx_packet pk[4] = {};
            for (int i = 0; i < 4; i++) {
                const auto p = udp4(dst[i], 9, 9);
                pk[i].in_off = arena.size();
                pk[i].len = 32;
                arena.insert(arena.end(), p.begin(), p.end());
            }
            while (!stop) {
                int32_t status[4];
                CHECK(neb_tx_resolve_batch_host(t, pk, 4, arena.data(), arena.size(), nullptr, status) == NEB_OK);
                CHECK(status[0] == NEB_STATUS_OK && pk[0].tunnel == 7);  // never a miss
                const uint32_t g = pk[1].tunnel;
                CHECK(g == 1 || g == 2);
                for (int i = 1; i < 4; i++) CHECK(status[i] == NEB_STATUS_OK && pk[i].tunnel == g);  // one route set
            }
        });
    for (auto& x : th) x.join();
    CHECK(neb_tx_table_destroy(t) == NEB_OK);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "threads") {
        threads();
        std::printf("route_test: ok (threads)\n");
        return 0;
    }
    neb_tx_table* t = nullptr;
    CHECK(neb_tx_table_create(nullptr, 32, 8, 8, &t) == NEB_OK);
    set_own(t);
    truncations(t);
    random_updates(t);
    CHECK(neb_tx_table_destroy(t) == NEB_OK);
    threads();
    std::printf("route_test: ok (exact, threads)\n");
    return 0;
}
