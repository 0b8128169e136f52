// peer_test.cpp — the peer table's rules, host table and host form (peer_core.hpp, peer.cpp) under
// sanitizers: a stand-alone program, no HIP.
//   (no argument)  exact: every truncation of a set of opened packets resolved from a heap buffer of
//                  exactly its length (header, plaintext and tag room: nothing past it is read);
//                  random updates (enough of them for the table to rebuild itself, which the
//                  program checks) against a linear-scan model, the batch in an arena that ends
//                  with its last packet; the same records kept as a device image through
//                  table_mirror.hpp on a fake device (updates in `first` / `second` order, a
//                  rebuild into the spare image) and searched there with peer_find; the threads once.
//                  The image part checks TableMirror, peer_find and tx_longest_prefix over an image
//                  that this program files itself (struct Image restates peer.cpp's policy: puts
//                  first, tombstones second, compaction at 3/4). peer.cpp's own device half is
//                  compiled out without HIP, so the order of the ops it emits is not checked here:
//                  tests/test_gpu_rx_inner.py does that on the device.
//   threads        two updating threads against two resolving ones: a steady entry never misses,
//                  and a replaced entry is seen with its old or its new type, never absent.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/nebula_aead.h"
#include "../../nebula_amd/csrc/peer_core.hpp"
#include "../../nebula_amd/csrc/table_mirror.hpp"

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::abort();                                             \
        }                                                             \
    } while (0)

namespace {

neb_cidr cidr4(uint32_t a, uint32_t bits) {
    neb_cidr c{};
    c.family = 4;
    c.bits = (uint8_t)bits;
    for (int i = 0; i < 4; i++) c.addr[i] = (uint8_t)(a >> (24 - 8 * i));
    return c;
}
neb_peer_net net4(uint32_t tunnel, uint32_t a, uint32_t bits, uint32_t type) { return neb_peer_net{tunnel, type, cidr4(a, bits)}; }
neb_peer_key key4(uint32_t tunnel, uint32_t a, uint32_t bits) { return neb_peer_key{tunnel, cidr4(a, bits)}; }

constexpr uint32_t kMe = 0x0A010007u;  // 10.1.0.7, the routable address
const uint64_t kEpoch[4] = {11, 22, 33, 44};

// An opened packet: header Message/None, a UDP/IPv4 packet from src to dst, 16 bytes of tag room.
std::vector<uint8_t> wire4(uint32_t src, uint32_t dst, uint64_t counter) {
    std::vector<uint8_t> w(16 + 32 + 16, 0);
    w[0] = 0x11;
    for (int i = 0; i < 8; i++) w[8 + i] = (uint8_t)(counter >> (56 - 8 * i));
    uint8_t* p = w.data() + 16;
    p[0] = 0x45, p[3] = 32, p[9] = 17;
    for (int i = 0; i < 4; i++) p[12 + i] = (uint8_t)(src >> (24 - 8 * i)), p[16 + i] = (uint8_t)(dst >> (24 - 8 * i));
    p[21] = 5, p[23] = 6;
    return w;
}

// One packet from a heap buffer of exactly its length.
int32_t inner_exact(neb_peer_table* t, const std::vector<uint8_t>& w, uint32_t key_id, neb_plain_packet* plain, neb_fw_packet* fw) {
    uint8_t* buf = (uint8_t*)std::malloc(w.size() ? w.size() : 1);
    if (!w.empty()) std::memcpy(buf, w.data(), w.size());
    neb_rx_packet pk{};
    pk.len = (uint32_t)w.size();
    pk.key_id = key_id;
    int32_t open = NEB_STATUS_OK, st = -1;
    CHECK(neb_rx_inner_batch_host(t, &pk, &open, kEpoch, 4, 1, buf, w.size(), plain, fw, &st) == NEB_OK);
    std::free(buf);
    return st;
}

void truncations(neb_peer_table* t) {
    std::vector<std::vector<uint8_t>> tpl;
    tpl.push_back(wire4(0x0A010009u, kMe, 7));
    {  // IHL 24, ICMP
        std::vector<uint8_t> w = wire4(0x0A010009u, kMe, 8);
        w[16] = 0x46, w[16 + 9] = 1;
        w.resize(16 + 40 + 16, 0);
        tpl.push_back(w);
    }
    {  // IPv6: hop-by-hop, routing, fragment (first), AH, destination options, then ICMPv6 echo
        std::vector<uint8_t> p(40, 0);
        p[0] = 0x60, p[6] = 0, p[8] = 0xfd, p[24] = 0xfd, p[39] = 9;
        const uint8_t next[] = {43, 44, 51, 60, 58};
        for (int k = 0; k < 5; k++) {
            std::vector<uint8_t> e(next[k] == 60 /* this one is the AH */ ? 12 : 8, 0);
            e[0] = next[k];
            if (e.size() == 12) e[1] = 1;
            p.insert(p.end(), e.begin(), e.end());
        }
        const uint8_t echo[8] = {128, 0, 0, 0, 0x12, 0x34, 0, 1};
        p.insert(p.end(), echo, echo + 8);
        for (int variant = 0; variant < 3; variant++) {
            std::vector<uint8_t> q = p;
            if (variant == 1) q[40 + 8 + 8 + 2] = 1;  // a non-first fragment
            if (variant == 2) q[41] = 255;            // an extension length past the end
            std::vector<uint8_t> w(16, 0);
            w[0] = 0x11;
            w.insert(w.end(), q.begin(), q.end());
            w.resize(w.size() + 16, 0);
            tpl.push_back(w);
        }
    }
    for (const auto& w : tpl)
        for (size_t cut = 0; cut <= w.size(); cut++) {
            neb_plain_packet plain;
            neb_fw_packet fw;
            const int32_t st = inner_exact(t, std::vector<uint8_t>(w.begin(), w.begin() + cut), 0, &plain, &fw);
            CHECK(st == NEB_STATUS_NOT_MESSAGE || st == NEB_STATUS_INVALID || st == NEB_STATUS_OK || st == NEB_STATUS_RX_BAD_REMOTE);
            CHECK((st == NEB_STATUS_NOT_MESSAGE) == (cut < 32));
            CHECK((st == NEB_STATUS_OK) == !(plain.flags & NEB_PLAIN_SKIP));
            if (st == NEB_STATUS_OK) CHECK(plain.off == 16 && plain.len == cut - 32 && (plain.flags & NEB_PLAIN_PARSED) && plain.epoch == 11);
        }
}

// ---- the model and the device image ---------------------------------------------------------------

using MKey = std::tuple<uint32_t, uint32_t, uint32_t>;  // tunnel, masked address, bits
struct Model {
    std::map<MKey, uint32_t> nets;
    static uint32_t mask(uint32_t bits) { return bits ? ~0u << (32 - bits) : 0u; }
    int32_t expect(uint32_t tunnel, uint32_t src, uint32_t dst) const {
        int best = -1;
        uint32_t type = 0;
        for (const auto& n : nets)
            if (std::get<0>(n.first) == tunnel && (src & mask(std::get<2>(n.first))) == std::get<1>(n.first) &&
                (int)std::get<2>(n.first) > best)
                best = (int)std::get<2>(n.first), type = n.second;
        if (best < 0) return NEB_STATUS_RX_BAD_REMOTE;
        if (type == NEB_NET_VPN_PEER) return NEB_STATUS_RX_PEER_REJECTED;
        return dst == kMe ? NEB_STATUS_OK : NEB_STATUS_RX_BAD_LOCAL;
    }
};

// A quiet fake device for table_mirror.hpp (tests/sanitize/mirror_test.cpp pins the mirror's own
// ordering rules from a logging one): host memory, events that do nothing.
struct Fake {
    using Stream = int;
    using Event = int*;
    using Error = int;
    static constexpr int kOk = 0;
    static constexpr unsigned kPinned = 0;
    static int event_create_host(Event* ev) { *ev = new int(0); return kOk; }
    static int event_sync(Event) { return kOk; }
    static int event_record(Event, Stream) { return kOk; }
    static void event_destroy(Event ev) { delete ev; }
    static int stream_wait(Stream, Event) { return kOk; }
    static int stream_sync(Stream) { return kOk; }
    static int device_sync() { return kOk; }
    static int memset(void* p, int v, size_t bytes) { std::memset(p, v, bytes); return kOk; }
    static int copy_h2d(void* dst, const void* src, size_t bytes, Stream) { std::memcpy(dst, src, bytes); return kOk; }
    static int mem_alloc(uint8_t** p, size_t bytes) { *p = (uint8_t*)std::malloc(bytes); return kOk; }
    static void mem_free(uint8_t* p) { std::free(p); }
    static int host_alloc(uint8_t** p, size_t bytes, unsigned) { return mem_alloc(p, bytes); }
    static void host_free(uint8_t* p) { std::free(p); }
};
struct Op {  // route.hpp's TxOp
    uint64_t slot, tag, addr_lo, addr_hi, value;
};
// route.hip's scatter, one op after the other: the record, then the tag.
int scatter(neb::TxSlot* image, const Op* ops, uint32_t n, int) {
    for (uint32_t i = 0; i < n; i++) {
        neb::TxSlot* s = image + ops[i].slot;
        if (ops[i].tag != neb::kTxTomb) s->value = ops[i].value, s->addr_lo = ops[i].addr_lo, s->addr_hi = ops[i].addr_hi;
        s->tag = ops[i].tag;
    }
    return Fake::kOk;
}

// The records as peer.cpp files them, kept beside a mirror: puts go into `first`, tombstones into `second`.
struct Image {
    std::vector<neb::TxSlot> host;
    uint32_t mask, used = 0;
    neb::TableMirror<Fake, neb::TxSlot, Op> dev;
    std::vector<Op> first, second;
    explicit Image(uint32_t cap) : host(neb::tx_slots_for(cap)), mask((uint32_t)host.size() - 1u) { CHECK(dev.init(host.size()) == NEB_OK); }
    static neb::TxAddr addr(uint32_t a, uint32_t bits) { return neb::TxAddr{(uint64_t)(a & Model::mask(bits)) << 32, 0}; }
    bool find(uint32_t tunnel, uint32_t a, uint32_t bits, uint32_t* s) {
        uint32_t probes;
        return neb::peer_find(host.data(), mask, tunnel, 4, bits, addr(a, bits), neb::HostLoad{}, s, &probes);
    }
    void del(uint32_t tunnel, uint32_t a, uint32_t bits) {
        uint32_t s;
        if (!find(tunnel, a, bits, &s)) return;
        host[s].tag = neb::kTxTomb;
        second.push_back(Op{s, neb::kTxTomb, 0, 0, 0});
    }
    void put(uint32_t tunnel, uint32_t a, uint32_t bits, uint32_t type) {
        const neb::TxAddr ad = addr(a, bits);
        const uint64_t h = neb::peer_hash(tunnel, 4, bits, ad);
        uint32_t old, s = (uint32_t)h & mask;
        const bool had = find(tunnel, a, bits, &old);
        while (host[s].tag != neb::kTxEmpty) s = (s + 1u) & mask;
        host[s] = neb::TxSlot{neb::peer_tag(tunnel, 4, bits, h), ad.lo, ad.hi, type};
        used++;
        first.push_back(Op{s, host[s].tag, ad.lo, ad.hi, type});
        if (had) {
            host[old].tag = neb::kTxTomb;
            second.push_back(Op{old, neb::kTxTomb, 0, 0, 0});
        }
    }
    void flush(const Model& m, int stream) {
        if (used > (mask + 1u) / 4u * 3u) {  // compaction: the live records into the spare image
            std::vector<neb::TxSlot> fresh(host.size());
            host.swap(fresh);
            used = 0;
            first.clear(), second.clear();
            for (const auto& n : m.nets) put(std::get<0>(n.first), std::get<1>(n.first), std::get<2>(n.first), n.second);
            first.clear(), second.clear();
            CHECK(dev.rebuild(host.data(), stream) == NEB_OK);
        } else {
            CHECK(dev.update(first, second, stream, scatter) == NEB_OK);
            first.clear(), second.clear();
        }
    }
    // the longest-prefix lookup over the active image, as the device form does it
    int32_t inner(uint32_t tunnel, uint32_t src, uint32_t dst, const neb::TxLens& lens) {
        int32_t st = -1;
        CHECK(dev.read(1, [&](int, const neb::TxSlot* image) {
            uint64_t type = 0;
            const bool found = neb::tx_longest_prefix(lens, 4, neb::TxAddr{(uint64_t)src << 32, 0}, [&](uint32_t bits, const neb::TxAddr& masked) {
                uint32_t s, probes;
                if (!neb::peer_find(image, mask, tunnel, 4, bits, masked, neb::HostLoad{}, &s, &probes)) return false;
                type = image[s].value;
                return true;
            });
            st = !found ? NEB_STATUS_RX_BAD_REMOTE : type == NEB_NET_VPN_PEER ? NEB_STATUS_RX_PEER_REJECTED
                 : dst == kMe ? NEB_STATUS_OK : NEB_STATUS_RX_BAD_LOCAL;
            return Fake::kOk;
        }) == NEB_OK);
        return st;
    }
};

void random_updates(neb_peer_table* t) {
    std::mt19937 rng(11);
    Model m;
    Image img(32);
    const uint32_t lengths[] = {0, 1, 8, 16, 24, 31, 32};
    auto pool = [&](uint32_t* a, uint32_t* bits, uint32_t* tunnel) {  // a small space, so keys recur
        *bits = lengths[rng() % 7];
        *a = (0x14000000u + ((rng() % 2) << 16) + ((rng() % 2) << 8) + rng() % 4) & Model::mask(*bits);
        *tunnel = rng() % 3;
    };
    const neb_peer_key hot = key4(3, 0x1E000000u, 24);
    uint32_t last_probes = 0, rebuilds = 0;
    for (int step = 0; step < 500; step++) {
        std::vector<neb_peer_key> del;
        std::vector<neb_peer_net> put;
        Model next = m;
        uint32_t a, bits, tunnel;
        if (step % 97 == 96)  // a burst over the capacity: refused whole
            for (uint32_t k = 0; k < 40; k++) {
                put.push_back(net4(2, 0x28000000u + (k << 8), 24, NEB_NET_UNSAFE));
                next.nets[MKey{2, 0x28000000u + (k << 8), 24}] = NEB_NET_UNSAFE;
            }
        for (uint32_t k = rng() % 4; k; k--) {
            pool(&a, &bits, &tunnel);
            del.push_back(key4(tunnel, a | (rng() & ~Model::mask(bits)), bits));  // host bits are ignored
            next.nets.erase(MKey{tunnel, a, bits});
        }
        for (uint32_t k = rng() % 5; k; k--) {
            pool(&a, &bits, &tunnel);
            const uint32_t type = 1 + rng() % 3;
            put.push_back(net4(tunnel, a | (rng() & ~Model::mask(bits)), bits, type));
            next.nets[MKey{tunnel, a, bits}] = type;
        }
        put.push_back(net4(3, 0x1E000000u, 24, 1 + (uint32_t)step % 3));  // replaced every step: its chain grows
        next.nets[MKey{3, 0x1E000000u, 24}] = 1 + (uint32_t)step % 3;
        const int rc = neb_peer_table_update(t, del.data(), (uint32_t)del.size(), put.data(), (uint32_t)put.size(), nullptr);
        if (next.nets.size() > 32) {
            CHECK(rc == NEB_ERR_NO_KEY_SLOT);  // and nothing applied
        } else {
            CHECK(rc == NEB_OK);
            m = next;
            for (const auto& d : del) img.del(d.tunnel, (uint32_t)d.prefix.addr[0] << 24 | d.prefix.addr[1] << 16 | d.prefix.addr[2] << 8 | d.prefix.addr[3], d.prefix.bits);
            for (const auto& p : put) img.put(p.tunnel, (uint32_t)p.prefix.addr[0] << 24 | p.prefix.addr[1] << 16 | p.prefix.addr[2] << 8 | p.prefix.addr[3], p.prefix.bits, p.type);
            img.flush(m, 1 + step % 3);
        }
        uint32_t probe[3], live;
        CHECK(neb_peer_table_probe(t, &hot, probe) == NEB_OK && probe[0] == 1);
        if (probe[2] < last_probes) rebuilds++;  // a chain only shrinks in a rebuild
        last_probes = probe[2];
        CHECK(neb_peer_table_count(t, &live) == NEB_OK && live == m.nets.size());
        neb::TxLens lens{};
        for (const auto& n : m.nets) neb::tx_lens_add(&lens, 4, std::get<2>(n.first));
        // a batch in an arena that ends with its last packet, at odd offsets
        const uint32_t n = 24, sz = 64;
        const size_t bytes = 1 + (size_t)n * (sz + 1) - 1;
        uint8_t* arena = (uint8_t*)std::malloc(bytes);
        std::memset(arena, 0xA5, bytes);
        std::vector<neb_rx_packet> pk(n);
        std::vector<uint32_t> src(n), dst(n);
        std::vector<int32_t> open(n, NEB_STATUS_OK), st(n);
        for (uint32_t i = 0; i < n; i++) {
            src[i] = i % 5 == 0 ? 0x1E000009u : 0x14000000u + ((rng() % 2) << 16) + ((rng() % 2) << 8) + rng() % 6;
            dst[i] = i % 7 == 3 ? kMe + 1 : kMe;
            const std::vector<uint8_t> w = wire4(src[i], dst[i], i);
            pk[i].off = 1 + (uint64_t)i * (sz + 1);
            pk[i].len = sz;
            pk[i].key_id = i % 5 == 0 ? 3 : rng() % 3;
            std::memcpy(arena + pk[i].off, w.data(), sz);
        }
        std::vector<neb_plain_packet> plain(n);
        std::vector<neb_fw_packet> fw(n);
        CHECK(neb_rx_inner_batch_host(t, pk.data(), open.data(), kEpoch, 4, n, arena, bytes, plain.data(), fw.data(), st.data()) == NEB_OK);
        CHECK(neb_rx_inner_batch_host(t, pk.data(), open.data(), kEpoch, 4, n, arena, bytes - 1, plain.data(), fw.data(), st.data()) == NEB_ERR_INVALID);
        for (uint32_t i = 0; i < n; i++) {
            CHECK(st[i] == m.expect(pk[i].key_id, src[i], dst[i]));
            CHECK(st[i] == img.inner(pk[i].key_id, src[i], dst[i], lens));  // the image answers as the host copy does
            CHECK(fw[i].remote_port == 5 && fw[i].local_port == 6 && fw[i].family == 4 && fw[i].ip_hdr_len == 20);
            CHECK((st[i] == NEB_STATUS_OK) == (plain[i].flags == NEB_PLAIN_PARSED) && (st[i] == NEB_STATUS_OK || plain[i].flags == NEB_PLAIN_SKIP));
        }
        std::free(arena);
    }
    CHECK(rebuilds >= 3);  // the updates alone rebuilt the table, and the model held across it
    img.dev.drain();
}

void threads() {
    neb_peer_table* t = nullptr;
    CHECK(neb_peer_table_create(nullptr, 32, &t) == NEB_OK);
    const neb_cidr me = cidr4(kMe, 32);
    CHECK(neb_peer_table_set_routable(t, &me, 1) == NEB_OK);
    const uint32_t steady = 0x0A010064u, swap = 0x0A010065u;
    const neb_peer_net base[2] = {net4(0, steady, 32, NEB_NET_VPN), net4(0, swap, 32, NEB_NET_VPN)};
    CHECK(neb_peer_table_update(t, nullptr, 0, base, 2, nullptr) == NEB_OK);
    std::atomic<bool> stop{false};
    std::vector<std::thread> th;
    th.emplace_back([&] {  // entries come, go and are replaced; the steady one is replaced by itself
        std::mt19937 rng(1);
        for (int k = 0; k < 4000; k++) {
            const neb_peer_key del = key4(1, 0x14000000u + (rng() % 20u << 8), 24);
            const neb_peer_net put[2] = {net4(1, 0x14000000u + (rng() % 20u << 8), 24, NEB_NET_UNSAFE), net4(0, steady, 32, NEB_NET_VPN)};
            CHECK(neb_peer_table_update(t, &del, 1, put, 2, nullptr) == NEB_OK);
        }
        stop = true;
    });
    th.emplace_back([&] {  // one entry flips between two types; the routable set is replaced by itself
        for (int k = 0; !stop; k++) {
            const neb_peer_net put = net4(0, swap, 32, k & 1 ? NEB_NET_VPN : NEB_NET_VPN_PEER);
            CHECK(neb_peer_table_update(t, nullptr, 0, &put, 1, nullptr) == NEB_OK);
            CHECK(neb_peer_table_set_routable(t, &me, 1) == NEB_OK);
        }
    });
    for (int r = 0; r < 2; r++)
        th.emplace_back([&] {
            std::vector<uint8_t> arena;
            neb_rx_packet pk[2] = {};
            const uint32_t src[2] = {steady, swap};
            for (int i = 0; i < 2; i++) {
                const auto w = wire4(src[i], kMe, 9);
                pk[i].off = arena.size();
                pk[i].len = (uint32_t)w.size();
                arena.insert(arena.end(), w.begin(), w.end());
            }
            const int32_t open[2] = {NEB_STATUS_OK, NEB_STATUS_OK};
            while (!stop) {
                int32_t st[2];
                neb_plain_packet plain[2];
                CHECK(neb_rx_inner_batch_host(t, pk, open, kEpoch, 4, 2, arena.data(), arena.size(), plain, nullptr, st) == NEB_OK);
                CHECK(st[0] == NEB_STATUS_OK);                                           // never a miss
                CHECK(st[1] == NEB_STATUS_OK || st[1] == NEB_STATUS_RX_PEER_REJECTED);  // the old or the new type
            }
        });
    for (auto& x : th) x.join();
    CHECK(neb_peer_table_destroy(t) == NEB_OK);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "threads") {
        threads();
        std::printf("peer_test: ok (threads)\n");
        return 0;
    }
    neb_peer_table* t = nullptr;
    CHECK(neb_peer_table_create(nullptr, 32, &t) == NEB_OK);
    const neb_cidr me = cidr4(kMe, 32);
    CHECK(neb_peer_table_set_routable(t, &me, 1) == NEB_OK);
    const neb_peer_net peer = net4(0, 0x0A010009u, 32, NEB_NET_VPN);
    CHECK(neb_peer_table_update(t, nullptr, 0, &peer, 1, nullptr) == NEB_OK);
    truncations(t);
    const neb_peer_key gone = key4(0, 0x0A010009u, 32);
    CHECK(neb_peer_table_update(t, &gone, 1, nullptr, 0, nullptr) == NEB_OK);
    random_updates(t);
    CHECK(neb_peer_table_destroy(t) == NEB_OK);
    threads();
    std::printf("peer_test: ok (exact, image, threads)\n");
    return 0;
}
