// recv_test.cpp — the RX receive plan's rules and host form (recv_core.hpp, recv.cpp) under ASan +
// UBSan: a stand-alone program, no HIP.
//   walk   the directed control buffers (truncated, corrupt and hostile cmsg lengths, a UDP_GRO
//          cmsg just past the end) and random ones, each at the very end of a heap allocation of
//          exactly its length, through recv_cmsg_walk and, as a one-entry batch, through the host
//          form, against the walk restated here;
//   exact  random batches planned from heap buffers of exactly their length into outputs of exactly
//          max_packets / nentries elements, against the loop restated here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/nebula_aead.h"
#include "../../nebula_amd/csrc/recv_core.hpp"

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::abort();                                             \
        }                                                             \
    } while (0)

namespace {

using namespace neb;
using Bytes = std::vector<uint8_t>;

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

// One control message: header, data, zero padding up to `space` bytes.
Bytes cmsg(int32_t level, int32_t type, const Bytes& data, uint64_t len, size_t space) {
    Bytes b(16 + data.size());
    std::memcpy(&b[0], &len, 8), std::memcpy(&b[8], &level, 4), std::memcpy(&b[12], &type, 4);
    if (!data.empty()) std::memcpy(&b[16], data.data(), data.size());
    b.resize(space);
    return b;
}
Bytes i32(int32_t v) {
    Bytes b(4);
    std::memcpy(b.data(), &v, 4);
    return b;
}
Bytes gro(int32_t v) { return cmsg(17, 104, i32(v), 20, 24); }
Bytes operator+(Bytes a, const Bytes& b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}

// parseRecvCmsg restated with explicit bounds: every read is checked against L first.
int32_t walk_ref(const Bytes& c, size_t L) {
    int32_t g = 0;
    size_t off = 0;
    CHECK(L <= c.size());
    while (off + 16 <= L) {
        int64_t len;
        int32_t level, type;
        std::memcpy(&len, &c[off], 8), std::memcpy(&level, &c[off + 8], 4), std::memcpy(&type, &c[off + 12], 4);
        if (len < 16 || len > (int64_t)(L - off)) return g;
        if (level == 17 && type == 104 && off + 20 <= L) std::memcpy(&g, &c[off + 16], 4);
        off += (size_t)((len + 7) & ~(int64_t)7);
    }
    return g;
}

// The buffer's first L bytes alone in an allocation of exactly L bytes: the walk itself, and the host
// form over a one-entry batch whose slot is that allocation (the stride says 1024, ctrl_len more).
void run_ctrl(const Bytes& c, size_t L, int32_t want) {
    CHECK(walk_ref(c, L) == want);
    Exact<uint8_t> buf(L);
    if (L) std::memcpy(buf.p, c.data(), L);
    uint8_t dummy[8] = {};
    CHECK(recv_cmsg_walk(L ? buf.p : dummy, (uint32_t)L) == want);
    if (!L) return;
    neb_recv_entry en{};
    en.off = 4096, en.len = 60000, en.seg_size = 3, en.ctrl_len = (uint32_t)L;
    const uint64_t cnt = recv_count(en.len, want);
    Exact<neb_rx_packet> pk(cnt);
    uint32_t first = 9, counts[2] = {9, 9};
    CHECK(neb_rx_recv_plan_host(&en, 1, buf.p, kRecvMaxCtrlStride, 1, pk.p, nullptr, nullptr, (uint32_t)cnt, nullptr, &first,
                                counts) == NEB_OK);
    CHECK(first == 0 && counts[0] == cnt && counts[1] == 1);
    CHECK(pk.p[cnt - 1].off + pk.p[cnt - 1].len == en.off + en.len && pk.p[0].key_id == NEB_KEYS_MIXED);
}

void walk_cases(std::mt19937& rng) {
    const Bytes tos = cmsg(0, 1, {0x2e}, 17, 24);
    run_ctrl(gro(1000), 0, 0);
    run_ctrl(gro(1000), 15, 0);
    run_ctrl(gro(1000), 16, 0);   // the header alone: its data is past the end
    run_ctrl(gro(1000), 19, 0);
    run_ctrl(gro(1000), 20, 1000);  // the cmsg without its padding
    run_ctrl(gro(1000), 24, 1000);
    run_ctrl(tos + gro(1000), 48, 1000);
    run_ctrl(tos + gro(1000), 44, 1000);
    run_ctrl(gro(1000) + gro(1500), 48, 1500);
    run_ctrl(gro(1000) + gro(1500), 24, 1000);  // the second lies just past the end
    run_ctrl(gro(1000) + gro(1500), 43, 1000);  // its length says 20, 19 are left
    run_ctrl(cmsg(17, 103, i32(1000), 20, 24), 24, 0);
    run_ctrl(cmsg(6, 104, i32(1000), 20, 24), 24, 0);
    run_ctrl(gro(1000) + cmsg(17, 104, i32(1500), 16, 24), 24 + 18, 1000);  // header-only cmsg, data 2 past the end
    run_ctrl(gro(-1400), 24, -1400);
    for (uint64_t len : {(uint64_t)15, (uint64_t)25, (uint64_t)0, ((uint64_t)1 << 63) - 8, (uint64_t)1 << 63, ~(uint64_t)0,
                         ((uint64_t)1 << 32) + 20, (uint64_t)1 << 20, (uint64_t)0x7FFFFFFFFFFFFFF7})
        run_ctrl(gro(1000) + cmsg(17, 104, i32(1500), len, 24), 48, 1000);
    // random: plausible headers with hostile lengths, every prefix length
    for (int it = 0; it < 4000; it++) {
        Bytes c;
        while (c.size() < 40 + rng() % 100) {
            const uint64_t lens[] = {16, 17, 20, 24, 15, 0, 32, rng() % 64, ~(uint64_t)0 - rng() % 9, (uint64_t)1 << 63, rng()};
            const uint64_t len = lens[rng() % 11];
            c = c + cmsg(rng() % 3 ? 17 : 0, rng() % 3 ? 104 : 1, i32((int32_t)rng()), len, 16 + 8 * (rng() % 4));
        }
        const size_t L = rng() % (c.size() + 1);
        run_ctrl(c, L, walk_ref(c, L));
    }
}

struct Batch {
    std::vector<neb_recv_entry> entries;
    Bytes ctrl;
    uint32_t stride, socket_v4, max_packets;
    bool use_ctrl;
};
struct Plan {
    std::vector<neb_rx_packet> pk;
    std::vector<neb_rx_source> src;
    std::vector<uint32_t> pkt_entry, first;
    std::vector<neb_udp_addr> from;
    uint32_t np = 0, done = 0;
};

// ListenOut's loop restated byte by byte.
Plan plan_ref(const Batch& b) {
    Plan p;
    uint64_t np = 0;
    bool cut = false;
    for (size_t j = 0; j < b.entries.size(); j++) {
        const neb_recv_entry& e = b.entries[j];
        neb_udp_addr f{};
        f.port = (uint16_t)(e.name[2] << 8 | e.name[3]);
        const uint8_t* ip = e.name + 8;
        bool mapped = ip[10] == 0xFF && ip[11] == 0xFF;
        for (int k = 0; k < 10; k++) mapped = mapped && ip[k] == 0;
        if (b.socket_v4) f.family = 4, std::memcpy(f.addr, e.name + 4, 4);
        else if (mapped) f.family = 4, std::memcpy(f.addr, ip + 12, 4);
        else f.family = 6, std::memcpy(f.addr, ip, 16);
        p.from.push_back(f);
        int32_t seg = e.seg_size;
        if (b.use_ctrl) {
            const size_t L = e.ctrl_len < b.stride ? e.ctrl_len : b.stride;
            seg = walk_ref(Bytes(b.ctrl.begin() + j * b.stride, b.ctrl.begin() + (j + 1) * b.stride), L);
        }
        const bool whole = seg <= 0 || (uint32_t)seg >= e.len;
        const uint64_t cnt = whole ? 1 : (e.len + (uint64_t)seg - 1) / (uint64_t)seg;
        if (cut || np + cnt > b.max_packets) {
            cut = true;
            p.first.push_back(NEB_RECV_NONE);
            continue;
        }
        p.first.push_back((uint32_t)np);
        neb_rx_source s{};
        std::memcpy(s.addr, f.addr, 16), s.family = f.family;
        for (uint64_t at = 0; whole ? at == 0 : at < e.len; at += whole ? 1 : (uint32_t)seg) {
            const uint64_t rest = e.len - at;
            p.pk.push_back(neb_rx_packet{e.off + at, whole || rest < (uint32_t)seg ? (uint32_t)rest : (uint32_t)seg, NEB_KEYS_MIXED});
            p.src.push_back(s);
            p.pkt_entry.push_back((uint32_t)j);
        }
        np += cnt;
        CHECK(p.pk.size() == np);
        p.done = (uint32_t)j + 1;
    }
    p.np = (uint32_t)np;
    while (p.pk.size() < b.max_packets) {
        p.pk.push_back(neb_rx_packet{0, 0, NEB_KEYS_MIXED});
        p.src.push_back(neb_rx_source{});
        p.pkt_entry.push_back(NEB_RECV_NONE);
    }
    return p;
}

Batch random_batch(std::mt19937& rng) {
    Batch b;
    const uint32_t strides[] = {8, 24, 32, 64, 1024};
    b.stride = strides[rng() % 5], b.socket_v4 = rng() % 2, b.use_ctrl = rng() % 2;
    const size_t n = rng() % 24;
    uint64_t total = 0;
    for (size_t j = 0; j < n; j++) {
        neb_recv_entry e{};
        const uint32_t lens[] = {0, 1, 1364, 4092, 65535, (uint32_t)(rng() % 3000)};
        e.off = ((uint64_t)rng() << 12) + rng() % 4096, e.len = lens[rng() % 6];
        const int32_t segs[] = {0, -1, 1, 1364, (int32_t)e.len, (int32_t)e.len + 1, (int32_t)e.len - 1, 50 + (int32_t)(rng() % 2000)};
        e.seg_size = segs[rng() % 8];
        if (e.len > 3000 && e.seg_size > 0 && e.seg_size < 50) e.seg_size = 50;
        for (auto& x : e.name) x = (uint8_t)rng();
        if (rng() % 2) {
            std::memset(e.name + 8, 0, 10), e.name[18] = e.name[19] = 0xFF;
            if (rng() % 3 == 0) e.name[8 + 9 + rng() % 3] ^= (uint8_t)(1u << rng() % 8);  // a neighbour of ::ffff:0:0/96
        }
        Bytes slot = rng() % 4 ? (rng() % 2 ? gro(e.seg_size) : cmsg(0, 1, {1}, 17, 24) + gro(e.seg_size)) : Bytes();
        while (rng() % 4 == 0 && slot.size() < b.stride) slot.push_back((uint8_t)rng());
        e.ctrl_len = rng() % 5 ? (uint32_t)slot.size() : (uint32_t)(rng() % (2 * b.stride));
        slot.resize(b.stride, 0xEE);
        b.ctrl = b.ctrl + slot;
        b.entries.push_back(e);
    }
    for (size_t j = 0; j < n; j++) {  // the packets of all entries, without expanding them
        int32_t seg = b.entries[j].seg_size;
        if (b.use_ctrl) {
            const size_t L = b.entries[j].ctrl_len < b.stride ? b.entries[j].ctrl_len : b.stride;
            seg = walk_ref(Bytes(b.ctrl.begin() + j * b.stride, b.ctrl.begin() + (j + 1) * b.stride), L);
        }
        total += recv_count(b.entries[j].len, seg);
    }
    CHECK(total < 200000);
    const uint32_t t = (uint32_t)total;
    const uint32_t caps[] = {t, 0u, t + (uint32_t)(rng() % 40), (uint32_t)(rng() % (t + 2)), t + 1u};
    b.max_packets = caps[rng() % 5];
    return b;
}

void exact(std::mt19937& rng) {
    unsigned cut = 0, split = 0, unmapped = 0;
    for (int it = 0; it < 1500; it++) {
        const Batch b = random_batch(rng);
        const Plan want = plan_ref(b);
        const size_t n = b.entries.size(), mp = b.max_packets;
        const bool optional = it % 4 != 0;
        Exact<neb_recv_entry> en(b.entries);
        Exact<uint8_t> ctrl(b.ctrl);
        Exact<neb_rx_packet> pk(mp);
        Exact<neb_rx_source> src(optional ? mp : 0);
        Exact<uint32_t> pe(optional ? mp : 0), first(n);
        Exact<neb_udp_addr> from(optional ? n : 0);
        // required pointers of zero elements: one element nobody may touch
        Exact<neb_rx_packet> pk1(1);
        Exact<uint32_t> first1(1);
        uint32_t counts[2] = {7, 7};
        CHECK(neb_rx_recv_plan_host(en.p, (uint32_t)n, b.use_ctrl ? ctrl.p : nullptr, b.stride, b.socket_v4, mp ? pk.p : pk1.p, src.p,
                                    pe.p, (uint32_t)mp, from.p, n ? first.p : first1.p, counts) == NEB_OK);
        CHECK(counts[0] == want.np && counts[1] == want.done);
        CHECK(!mp || !std::memcmp(pk.p, want.pk.data(), mp * sizeof(neb_rx_packet)));
        CHECK(!n || !std::memcmp(first.p, want.first.data(), n * 4));
        if (optional) {
            CHECK(!mp || !std::memcmp(src.p, want.src.data(), mp * sizeof(neb_rx_source)));
            CHECK(!mp || !std::memcmp(pe.p, want.pkt_entry.data(), mp * 4));
            CHECK(!n || !std::memcmp(from.p, want.from.data(), n * sizeof(neb_udp_addr)));
        }
        CHECK(pk1.p[0].key_id == 0xA5A5A5A5u && first1.p[0] == 0xA5A5A5A5u);
        cut += want.done < n;
        split += want.np > want.done;
        for (const auto& f : want.from) unmapped += !b.socket_v4 && f.family == 4;
    }
    CHECK(cut > 100 && split > 100 && unmapped > 100);
    // argument errors
    neb_recv_entry e{};
    neb_rx_packet pk[2];
    uint32_t first[1], counts[2];
    uint8_t ctrl[64] = {};
    CHECK(neb_rx_recv_plan_host(&e, 1, nullptr, 0, 1, pk, nullptr, nullptr, 2, nullptr, first, counts) == NEB_OK);
    CHECK(neb_rx_recv_plan_host(nullptr, 1, nullptr, 0, 1, pk, nullptr, nullptr, 2, nullptr, first, counts) == NEB_ERR_INVALID);
    CHECK(neb_rx_recv_plan_host(&e, 1, nullptr, 0, 1, nullptr, nullptr, nullptr, 2, nullptr, first, counts) == NEB_ERR_INVALID);
    CHECK(neb_rx_recv_plan_host(&e, 1, nullptr, 0, 1, pk, nullptr, nullptr, 2, nullptr, nullptr, counts) == NEB_ERR_INVALID);
    CHECK(neb_rx_recv_plan_host(&e, 1, nullptr, 0, 1, pk, nullptr, nullptr, 2, nullptr, first, nullptr) == NEB_ERR_INVALID);
    CHECK(neb_rx_recv_plan_host(&e, 0x80000000u, nullptr, 0, 1, pk, nullptr, nullptr, 2, nullptr, first, counts) == NEB_ERR_INVALID);
    CHECK(neb_rx_recv_plan_host(&e, 1, nullptr, 0, 1, pk, nullptr, nullptr, 0x80000000u, nullptr, first, counts) == NEB_ERR_INVALID);
    for (uint32_t stride : {0u, 4u, 20u, 1032u})
        CHECK(neb_rx_recv_plan_host(&e, 1, ctrl, stride, 1, pk, nullptr, nullptr, 2, nullptr, first, counts) == NEB_ERR_INVALID);
}

}  // namespace

int main() {
    std::mt19937 rng(20261021);
    walk_cases(rng);
    exact(rng);
    std::printf("recv_test: ok (walk, exact)\n");
    return 0;
}
