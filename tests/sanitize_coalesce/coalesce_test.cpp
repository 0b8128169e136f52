// coalesce_test.cpp — coalesce_core.hpp and the host form (nebula_amd/csrc/coalesce.cpp) under
// ASan + UBSan: a stand-alone program, no HIP and no GPU. It fuzzes the parsers on exact-size heap
// buffers (an over-read is an ASan report), runs a randomised batch through
// neb_rx_coalesce_batch_host and checks its invariants, then the capacity cuts against the full run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../nebula_amd/csrc/coalesce_core.hpp"

using namespace neb;

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::abort();                                             \
        }                                                             \
    } while (0)

static bool same(const void* a, const void* b, size_t n) { return n == 0 || !std::memcmp(a, b, n); }
static std::mt19937 rng(12345);
static uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0; }

struct Flow {
    bool tcp, v6, df;
    uint16_t sport, id;
    uint32_t seq, size;
};

static std::vector<uint8_t> build(Flow& f, uint32_t pay, uint8_t flags, bool frag, bool opts) {
    const uint32_t ip = f.v6 ? 40 : (opts ? 24 : 20), l4 = f.tcp ? 20 : 8;
    std::vector<uint8_t> p(ip + l4 + pay, 0);
    if (f.v6) {
        p[0] = 0x60;
        co_put16(&p[4], l4 + pay);
        p[6] = f.tcp ? 6 : 17;
        p[7] = 64;
        p[23] = 1;
        p[39] = 2;
    } else {
        p[0] = 0x40 | (ip / 4);
        co_put16(&p[2], ip + l4 + pay);
        co_put16(&p[4], f.id++);
        co_put16(&p[6], (f.df ? 0x4000 : 0) | (frag ? 0x2000 : 0));
        p[8] = 64;
        p[9] = f.tcp ? 6 : 17;
        p[12] = 10;
        p[15] = 1;
        p[16] = 10;
        p[19] = 2;
    }
    co_put16(&p[ip], f.sport);
    co_put16(&p[ip + 2], 80);
    if (f.tcp) {
        p[ip + 4] = (uint8_t)(f.seq >> 24);
        p[ip + 5] = (uint8_t)(f.seq >> 16);
        p[ip + 6] = (uint8_t)(f.seq >> 8);
        p[ip + 7] = (uint8_t)f.seq;
        p[ip + 12] = 5 << 4;
        p[ip + 13] = flags;
        f.seq += pay;
    } else {
        co_put16(&p[ip + 4], 8 + pay);
    }
    for (uint32_t i = 0; i < pay; i++) p[ip + l4 + i] = (uint8_t)rng();
    return p;
}

struct Batch {
    std::vector<neb_plain_packet> plain;
    std::vector<uint8_t> arena;
};

static Batch random_batch(uint32_t n) {
    std::vector<Flow> flows;
    for (uint32_t f = 0; f < 24; f++)
        flows.push_back(Flow{f % 3 != 2, f % 4 == 1, f % 2 == 0, (uint16_t)(1000 + f), (uint16_t)rng(), (uint32_t)rng(),
                             f % 5 == 0 ? 100u : 1300u});
    Batch b;
    uint64_t ctr = 0;
    while (b.plain.size() < n) {
        Flow& f = flows[rnd((uint32_t)flows.size())];
        for (uint32_t k = rnd(90) + 1; k && b.plain.size() < n; k--) {
            const uint32_t x = rnd(100);
            uint32_t pay = f.size;
            uint8_t fl = kCoTcpAck;
            if (x < 3) fl |= kCoTcpPsh;
            if (x == 3) fl |= 1;
            if (x == 4) fl |= kCoTcpEce;
            if (x < 12 && x >= 6) pay = rnd(f.size);
            if (x == 12) f.seq += 5;
            if (x == 13) f.id += 9;
            std::vector<uint8_t> p = build(f, pay, fl, x == 14, x == 15);
            if (x == 16) p.resize(rnd((uint32_t)p.size()));  // a runt
            neb_plain_packet pp{};
            pp.off = b.arena.size();
            pp.len = (uint32_t)p.size();
            pp.epoch = 1 + rnd(2);
            pp.counter = ++ctr ^ (rnd(20) == 0 ? 3 : 0);  // a little reorder
            pp.flags = x == 17 ? NEB_PLAIN_SKIP : 0;
            b.arena.insert(b.arena.end(), p.begin(), p.end());
            b.plain.push_back(pp);
        }
    }
    return b;
}

struct Result {
    int rc;
    uint32_t nw;
    std::vector<neb_tun_write> writes;
    std::vector<uint8_t> out;
    std::vector<uint32_t> pw;
    std::vector<int32_t> ps;
};

static Result run(const Batch& b, size_t out_cap, uint32_t max_writes, uint32_t lanes) {
    Result r;
    const uint32_t n = (uint32_t)b.plain.size();
    r.writes.resize(max_writes);  // exact sizes: an overrun is an ASan report
    r.out.resize(out_cap);
    r.pw.resize(n);
    r.ps.resize(n);
    r.nw = 0;
    r.rc = neb_rx_coalesce_batch_host(b.plain.data(), n, b.arena.data(), b.arena.size(), r.out.data(), out_cap,
                                      r.writes.data(), max_writes, &r.nw, r.pw.data(), r.ps.data(), lanes);
    return r;
}

static void fuzz_parsers() {
    for (int it = 0; it < 200000; it++) {
        const uint32_t len = rnd(it % 7 == 0 ? 200 : 70);
        std::vector<uint8_t> p(len);
        for (auto& x : p) x = (uint8_t)rng();
        if (len && it % 2) p[0] = (it % 4 == 1 ? 0x45 : 0x60) | (p[0] & (it % 4 == 1 ? 0x03 : 0));
        if (len > 6 && it % 3 == 0) p[6] = (uint8_t)(it % 9 == 0 ? 44 : it % 9 == 3 ? 51 : it % 9 == 6 ? 0 : 6);
        if (len > 41 && it % 5 == 0) p[41] = (uint8_t)rnd(3);
        CoFw fw;
        const bool ok = co_new_packet(p.data(), len, &fw);
        neb_plain_packet pp{};
        pp.len = len;
        for (uint32_t lanes = 0; lanes < 4; lanes += 3) {
            CoRec r;
            co_classify(pp, p.data(), lanes, &r);
            CHECK((r.status == NEB_STATUS_OK) == ok);
            if (ok && r.cls != kCoPass && r.cls != kCoUnparse) CHECK(r.info.hdr_len + (r.cls == kCoSeal ? 0 : r.info.pay_len) <= len);
        }
        pp.flags = NEB_PLAIN_PARSED;
        pp.proto = it % 2 ? 6 : 17;
        pp.ip_hdr_len = (uint16_t)(it % 3 == 0 ? 20 : it % 3 == 1 ? 40 : rnd(70));
        CoRec r;
        co_classify(pp, p.data(), 3, &r);
        if (r.status == NEB_STATUS_OK && (r.cls == kCoData || r.cls == kCoAck))
            CHECK((uint32_t)r.info.hdr_len + r.info.pay_len <= len);
    }
}

static void check_batch(const Batch& b, const Result& r, uint32_t lanes) {
    const uint32_t n = (uint32_t)b.plain.size();
    CHECK(r.rc == NEB_OK);
    std::vector<uint32_t> carried(r.nw, 0);
    std::vector<uint64_t> paysum(r.nw, 0);
    for (uint32_t i = 0; i < n; i++) {
        CoRec rec;
        co_classify(b.plain[i], b.arena.data() + b.plain[i].off, lanes, &rec);
        if (rec.status != NEB_STATUS_OK) {
            CHECK(r.ps[i] == rec.status && r.pw[i] == NEB_WRITE_NONE);
            continue;
        }
        if (r.ps[i] == NEB_STATUS_NO_SPACE) {
            CHECK(r.pw[i] == NEB_WRITE_NONE);
            continue;
        }
        CHECK(r.ps[i] == NEB_STATUS_OK && r.pw[i] < r.nw);
        carried[r.pw[i]]++;
        paysum[r.pw[i]] += rec.info.pay_len;
    }
    uint64_t off = 0;
    for (uint32_t k = 0; k < r.nw; k++) {
        const neb_tun_write& w = r.writes[k];
        CHECK(w.out_off == off && w.nseg == carried[k] && w.out_off + w.len <= r.out.size());
        CHECK(k == 0 || w.lane >= r.writes[k - 1].lane);
        const neb_plain_packet& f = b.plain[w.first];
        if (w.nseg == 1) {
            CHECK(w.vnet_flags == NEB_VNET_F_DATA_VALID && w.gso_type == 0 && w.len == f.len);
            CHECK(!std::memcmp(r.out.data() + off, b.arena.data() + f.off, w.len));
        } else {
            CHECK(w.vnet_flags == NEB_VNET_F_NEEDS_CSUM && w.nseg <= kCoMaxSegs && w.len <= kCoBufSize);
            CHECK(w.len == w.hdr_len + paysum[k] && w.gso_size * (uint64_t)(w.nseg - 1) < paysum[k]);
            CHECK(paysum[k] <= (uint64_t)w.gso_size * w.nseg);
        }
        off += co_align16(w.len);
    }
}

int main() {
    CHECK(co_fold_once_no_invert(0) == 0 && co_fold_once_no_invert(0xFFFF) == 0xFFFF);
    CHECK(co_fold_once_no_invert(0x1FFFE) == 0xFFFF && co_fold_once_no_invert(0x10000) == 1);
    CHECK(co_fold_once_no_invert(0xFFFFFFFFu) == 0xFFFF);
    fuzz_parsers();
    const Batch b = random_batch(6000);
    size_t cap = 0;
    for (const auto& p : b.plain) cap += co_align16(p.len);
    uint32_t chains = 0;
    for (uint32_t lanes = 0; lanes < 4; lanes++) {
        const Result full = run(b, cap, (uint32_t)b.plain.size(), lanes);
        check_batch(b, full, lanes);
        for (uint32_t k = 0; k < full.nw; k++) chains += full.writes[k].nseg >= 2;
        // capacity cuts: the emitted prefix is the full run's
        const uint32_t cuts[] = {0, 1, full.nw / 3, full.nw - 1, full.nw};
        for (uint32_t mw : cuts) {
            const Result r = run(b, cap, mw, lanes);
            check_batch(b, r, lanes);
            CHECK(r.nw == mw && same(r.writes.data(), full.writes.data(), mw * sizeof(neb_tun_write)));
        }
        const size_t mid = full.writes[full.nw / 2].out_off;
        const size_t caps[] = {0, 15, mid - 1, mid, mid + 16, cap - 1};
        for (size_t c : caps) {
            const Result r = run(b, c, (uint32_t)b.plain.size(), lanes);
            check_batch(b, r, lanes);
            uint32_t want = 0;
            while (want < full.nw && full.writes[want].out_off + co_align16(full.writes[want].len) <= c) want++;
            CHECK(r.nw == want && same(r.out.data(), full.out.data(), want ? full.writes[want - 1].out_off : 0));
        }
    }
    CHECK(chains > 100);
    // bad arguments
    Batch bad = b;
    bad.plain[5].len = (uint32_t)bad.arena.size();
    CHECK(run(bad, cap, 10, 3).rc == NEB_ERR_INVALID);
    CHECK(run(b, cap, 10, 8).rc == NEB_ERR_INVALID);
    // wire to plain
    std::vector<uint8_t> wire(16 + 40 + 16, 0);
    wire[0] = 0x11;
    wire[15] = 9;
    neb_rx_packet pk{0, (uint32_t)wire.size(), 1};
    const int32_t st = NEB_STATUS_OK;
    const uint64_t epoch[2] = {5, 6};
    neb_plain_packet pl;
    CHECK(neb_rx_plain_from_wire_host(&pk, &st, epoch, 2, 1, wire.data(), wire.size(), &pl) == NEB_OK);
    CHECK(pl.flags == 0 && pl.off == 16 && pl.len == 40 && pl.counter == 9 && pl.epoch == 6);
    pk.key_id = 2;
    CHECK(neb_rx_plain_from_wire_host(&pk, &st, epoch, 2, 1, wire.data(), wire.size(), &pl) == NEB_OK);
    CHECK(pl.flags == NEB_PLAIN_SKIP);
    pk.len = (uint32_t)wire.size() + 1;
    CHECK(neb_rx_plain_from_wire_host(&pk, &st, epoch, 2, 1, wire.data(), wire.size(), &pl) == NEB_ERR_INVALID);
    std::printf("coalesce_test: ok\n");
    return 0;
}
