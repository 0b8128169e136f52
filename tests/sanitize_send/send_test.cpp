// send_test.cpp — the TX send plan's rules and host form (send_core.hpp, send.cpp) under ASan + UBSan:
// a stand-alone program, no HIP.
//   exact     random batches (sizes at the caps, shrinking sizes, 1 to 3 destinations, some
//             unroutable, bad indexes, NOT_SENT wires, max_segments 0 to 63 and 1024, chunks 0 to 128)
//             planned from heap buffers of exactly their length into heap buffers of exactly nwires
//             elements, against the packing loop restated here run by run (plan_run below);
//   parallel  the same batches through send_core.hpp's boundary predicate and plateau function, the
//             way the device form composes them, against the same loop.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/nebula_aead.h"
#include "../../nebula_amd/csrc/send_core.hpp"

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::abort();                                             \
        }                                                             \
    } while (0)

namespace {

using namespace neb;

template <class T>
struct Exact {  // a heap buffer of exactly n elements (n == 0: a null pointer)
    T* p;
    size_t n;
    explicit Exact(size_t n_) : p(n_ ? (T*)std::malloc(n_ * sizeof(T)) : nullptr), n(n_) { CHECK(!n_ || p); }
    explicit Exact(const std::vector<T>& v) : Exact(v.size()) {
        if (n) std::memcpy(p, v.data(), n * sizeof(T));
    }
    ~Exact() { std::free(p); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
};

struct Batch {
    std::vector<neb_tx_wire> wires;
    std::vector<int32_t> status;
    std::vector<neb_tx_packet> packets;
    std::vector<neb_relay_route> via;
    std::vector<neb_udp_addr> remote;
    bool with_via;
    uint32_t socket_v4, max_segments, chunk;
};
struct Plan {
    std::vector<neb_send_iov> iov;
    std::vector<neb_send_entry> entries;
    std::vector<uint32_t> wire_entry;
    std::vector<int32_t> send_status;
};

neb_udp_addr addr(uint8_t family, uint8_t last, uint16_t port, bool mapped = false) {
    neb_udp_addr a{};
    a.family = family, a.port = port;
    if (family == 4) a.addr[0] = 10, a.addr[3] = last;
    if (family == 6) {
        if (mapped) a.addr[10] = a.addr[11] = 0xFF, a.addr[12] = 10;
        else a.addr[0] = 0x20, a.addr[1] = 0x01;
        a.addr[15] = last;
    }
    return a;
}

Batch random_batch(std::mt19937& g) {
    auto pick = [&](uint32_t n) { return (uint32_t)(g() % n); };
    Batch b;
    b.remote = {addr(4, 1, 4242), addr(4, 2, 4242), addr(4, 1, 4243), addr(6, 1, 9999), addr(6, 9, 4242, true), addr(0, 0, 0),
                addr(4, 7, 4242), addr(0, 0, 0)};
    const uint32_t nt = (uint32_t)b.remote.size();
    b.via.assign(nt, neb_relay_route{NEB_RELAY_NONE, 0});
    b.via[7].tunnel = 6;
    b.with_via = pick(8) != 0;
    b.socket_v4 = pick(3) != 0;
    const uint32_t segs[] = {0, 1, 2, 3, 4, 7, 63, 1024}, chunks[] = {0, 1, 2, 3, 5, 8, 128};
    b.max_segments = segs[pick(8)];
    b.chunk = chunks[pick(7)];
    const uint32_t sizes[4][5] = {{0, 1, 65000, 65001, 1200}, {1200, 1200, 1200, 600, 600}, {32500, 21667, 13000, 1300, 30000},
                                  {100, 99, 98, 97, 1}};
    const uint32_t fam = pick(4), ndst = 1 + pick(3), n = pick(70);
    uint32_t pool[3] = {pick(nt), pick(nt), pick(nt)};
    uint32_t len = sizes[fam][pick(5)], dst = pool[pick(ndst)];
    uint64_t off = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t r = pick(100);
        if (r < 25) len = sizes[fam][pick(5)];
        else if (r < 40 && len) len -= pick(2);
        if (pick(100) < 15) dst = pool[pick(ndst)];
        neb_tx_packet pk{};
        pk.tunnel = pick(50) ? dst : nt + pick(3);
        b.packets.push_back(pk);
        neb_tx_wire w{};
        w.out_off = off, w.len = len, w.counter = i;
        w.packet = pick(60) ? (uint32_t)b.packets.size() - 1u : (uint32_t)b.packets.size() + pick(2);
        w.reserved = (dst == 7 || !pick(40)) ? NEB_TX_WIRE_VIA : 0;
        off += (len + 15u) & ~15ull;
        b.wires.push_back(w);
        b.status.push_back(pick(10) ? NEB_STATUS_OK : NEB_STATUS_EXHAUSTED);
    }
    return b;
}

// ---- the packing loop, restated: bufs with addresses, planRun, the chunk's iovec budget ----------
struct Buf {
    uint32_t wire, len, dst;
    int32_t status;
    neb_udp_addr a;
    bool own;  // a destination no other wire has
};
bool same_addr(const Buf& x, const Buf& y) { return !x.own && !y.own && !std::memcmp(&x.a, &y.a, sizeof(neb_udp_addr)); }

Plan plan_ref(const Batch& b) {
    const uint32_t n = (uint32_t)b.wires.size(), nt = (uint32_t)b.remote.size();
    Plan p;
    p.wire_entry.assign(n, NEB_SEND_NONE);
    p.send_status.assign(n, NEB_STATUS_NOT_SENT);
    std::vector<Buf> bufs;
    for (uint32_t i = 0; i < n; i++) {
        if (b.status[i] != NEB_STATUS_OK) continue;
        Buf f{i, b.wires[i].len, NEB_SEND_NONE, NEB_STATUS_BAD_KEY, neb_udp_addr{}, true};
        uint32_t t = b.wires[i].packet < b.packets.size() ? b.packets[b.wires[i].packet].tunnel : nt;
        if (t < nt && (b.wires[i].reserved & NEB_TX_WIRE_VIA)) t = b.with_via ? b.via[t].tunnel : nt;
        if (t < nt) {
            f.a = b.remote[t], f.own = false, f.dst = t;
            const bool mapped = f.a.family == 6 && !std::memcmp(f.a.addr, "\0\0\0\0\0\0\0\0\0\0\xff\xff", 12);
            f.status = f.a.family == 4 || (f.a.family == 6 && (!b.socket_v4 || mapped)) ? NEB_STATUS_OK : NEB_STATUS_UNROUTABLE;
        }
        p.send_status[i] = f.status;
        bufs.push_back(f);
    }
    const bool gso = b.max_segments > 1;
    size_t i = 0;
    while (i < bufs.size()) {
        uint32_t iov_idx = 0;
        while (i < bufs.size()) {
            const uint64_t budget = b.chunk ? b.chunk - iov_idx : bufs.size();
            if (budget < 1) break;
            // planRun
            const uint32_t seg = bufs[i].len;
            uint32_t run = 1;
            if (gso && seg != 0 && seg <= NEB_SEND_MAX_BYTES) {
                const uint64_t max_len = budget < b.max_segments ? budget : b.max_segments;
                uint64_t total = seg;
                while (run < max_len && i + run < bufs.size()) {
                    const Buf& nx = bufs[i + run];
                    if (nx.len == 0 || nx.len > seg || !same_addr(nx, bufs[i]) || total + nx.len > NEB_SEND_MAX_BYTES) break;
                    total += nx.len;
                    run++;
                    if (nx.len < seg) break;
                }
            }
            if (bufs[i].status != NEB_STATUS_OK) {
                i += run;
                continue;
            }
            neb_send_entry e{(uint32_t)p.iov.size(), (uint16_t)run, (uint16_t)(run >= 2 ? seg : 0), bufs[i].dst, 0};
            for (uint32_t k = 0; k < run; k++) {
                const Buf& f = bufs[i + k];
                p.iov.push_back(neb_send_iov{b.wires[f.wire].out_off, f.len, f.wire});
                p.wire_entry[f.wire] = (uint32_t)p.entries.size();
                e.bytes += f.len;
            }
            p.entries.push_back(e);
            i += run;
            iov_idx += run;
        }
    }
    return p;
}

// ---- the host form on exact-size buffers ----------------------------------------------------------
Plan plan_host(const Batch& b) {
    const uint32_t n = (uint32_t)b.wires.size();
    Exact<neb_tx_wire> wires(b.wires);
    Exact<int32_t> status(b.status);
    Exact<neb_tx_packet> packets(b.packets);
    Exact<neb_relay_route> via(b.via);
    Exact<neb_udp_addr> remote(b.remote);
    Exact<neb_send_iov> iov(n);
    Exact<neb_send_entry> entries(n);
    Exact<uint32_t> wire_entry(n);
    Exact<int32_t> send_status(n);
    Exact<uint32_t> counts(2);
    CHECK(neb_tx_send_plan_host(wires.p, status.p, n, packets.p, (uint32_t)packets.n, b.with_via ? via.p : nullptr, remote.p,
                                (uint32_t)remote.n, b.socket_v4, b.max_segments, b.chunk, iov.p, &counts.p[0], entries.p,
                                &counts.p[1], wire_entry.p, send_status.p) == NEB_OK);
    Plan p;
    CHECK(counts.p[0] <= n && counts.p[1] <= counts.p[0]);
    if (counts.p[0]) p.iov.assign(iov.p, iov.p + counts.p[0]);
    if (counts.p[1]) p.entries.assign(entries.p, entries.p + counts.p[1]);
    if (n) p.wire_entry.assign(wire_entry.p, wire_entry.p + n);
    if (n) p.send_status.assign(send_status.p, send_status.p + n);
    return p;
}

// ---- send_core.hpp's predicates composed as the device form composes them -------------------------
Plan plan_parallel(const Batch& b) {
    const uint32_t n = (uint32_t)b.wires.size();
    Plan p;
    p.wire_entry.assign(n, NEB_SEND_NONE);
    p.send_status.assign(n, 0);
    std::vector<SendRec> rec(n);
    std::vector<uint32_t> last(n), rank(n), flags(n, 0), ps(n, 0), fn(n), st(n, 0);
    uint32_t l = 0, r = 0;
    for (uint32_t i = 0; i < n; i++) {
        send_classify(b.wires[i], b.status[i], b.packets.data(), (uint32_t)b.packets.size(), b.with_via ? b.via.data() : nullptr,
                      b.remote.data(), (uint32_t)b.remote.size(), b.socket_v4, &rec[i]);
        p.send_status[i] = send_status_of(rec[i].cls);
        last[i] = l, rank[i] = r;
        if (rec[i].cls != kSendAbsent) l = i + 1;
        if (rec[i].cls == kSendRoutable) r++;
    }
    uint32_t run_ps = 0, acc = kSendFnIdentity, e = 0;
    std::vector<uint32_t> first;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t f = kSendFnIdentity;
        if (rec[i].cls == kSendRoutable) {
            const SendRec* pv = last[i] ? &rec[last[i] - 1] : &rec[i];
            if (send_hard(last[i] != 0, *pv, rec[i], rank[i], b.chunk)) flags[i] = 3;
            else if (pv->len != rec[i].len) flags[i] = 2;
            if (flags[i] & 1) f = kSendFnZero;
            else if (flags[i]) f = send_plateau_fn(rank[i] - ps[last[i] - 1], pv->len, rec[i].len, b.max_segments);
            if (flags[i]) run_ps = rank[i];
        }
        ps[i] = run_ps;
        acc = send_fn_compose(acc, f);
        fn[i] = acc;
        if (rec[i].cls != kSendRoutable) continue;
        st[i] = send_run_start(rank[i] - ps[i], fn[i] & 1u, send_run_cap(rec[i].len, b.max_segments));
        if (st[i]) first.push_back(i), e++;
        p.wire_entry[i] = e - 1;
        p.iov.push_back(neb_send_iov{b.wires[i].out_off, rec[i].len, i});
    }
    for (uint32_t k = 0; k < e; k++) {
        const uint32_t f0 = rank[first[k]], end = k + 1 < e ? rank[first[k + 1]] : r, cnt = end - f0;
        uint32_t bytes = 0;
        for (uint32_t q = f0; q < end; q++) bytes += p.iov[q].len;
        p.entries.push_back(neb_send_entry{f0, (uint16_t)cnt, (uint16_t)(cnt >= 2 ? p.iov[f0].len : 0), rec[first[k]].dst, bytes});
    }
    return p;
}

template <class T>
bool same(const std::vector<T>& x, const std::vector<T>& y) {
    return x.size() == y.size() && (x.empty() || !std::memcmp(x.data(), y.data(), x.size() * sizeof(T)));
}
void check_same(const Plan& x, const Plan& y) {
    CHECK(same(x.send_status, y.send_status));
    CHECK(same(x.wire_entry, y.wire_entry));
    CHECK(same(x.iov, y.iov));
    CHECK(same(x.entries, y.entries));
}

}  // namespace

int main() {
    std::mt19937 g(20261021);
    uint32_t runs = 0, absorbed = 0, skipped = 0;
    for (int it = 0; it < 20000; it++) {
        const Batch b = random_batch(g);
        const Plan ref = plan_ref(b);
        check_same(plan_host(b), ref);
        check_same(plan_parallel(b), ref);
        for (const auto& e : ref.entries) {
            runs += e.niov >= 2;
            absorbed += e.niov >= 2 && e.bytes != (uint32_t)e.niov * e.seg_size;
        }
        for (int32_t s : ref.send_status) skipped += s == NEB_STATUS_UNROUTABLE;
    }
    CHECK(runs > 1000 && absorbed > 100 && skipped > 1000);
    // argument errors
    uint32_t c[2];
    CHECK(neb_tx_send_plan_host(nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, 1, 1025, 128, nullptr, &c[0], nullptr, &c[1],
                                nullptr, nullptr) == NEB_ERR_INVALID);
    CHECK(neb_tx_send_plan_host(nullptr, nullptr, 1, nullptr, 0, nullptr, nullptr, 0, 1, 63, 128, nullptr, &c[0], nullptr, &c[1],
                                nullptr, nullptr) == NEB_ERR_INVALID);
    CHECK(neb_tx_send_plan_host(nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, 1, 63, 128, nullptr, &c[0], nullptr, &c[1],
                                nullptr, nullptr) == NEB_OK && c[0] == 0 && c[1] == 0);
    std::printf("send_test: ok (exact, parallel)\n");
    return 0;
}
