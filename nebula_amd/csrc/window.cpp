// window.cpp — the receive-side anti-replay window and the batched RX open that drives it
// (include/nebula_aead.h, "replay window + batched receive").
//
// WindowCore restates nebula.Bits (bits.go:15-262): a power-of-two circular bitmap of seen
// counters, slot 0 seeded so counter 0 reads as received (:47-48), Check (:134-150), Update with
// its fast path (:168-186) and slow path (:188-262: jump with lost accounting, in-window backfill
// or duplicate, out of window). Arithmetic is uint64 with wraparound, as in Go.
//
// neb_rx_open_batch_host is ConnectionState.Decrypt (connection_state.go:99-119) for a whole
// receive batch, with results identical to running it packet by packet in arrival order:
//   1. sequential simulation on private copies of the touched windows, assuming every tag
//      verifies: a packet the simulation refuses (replay, duplicate inside the batch, out of
//      window) is held back; the rest go to the GPU in one batch;
//   2. the real windows, in arrival order: Check, then the GPU's tag verdict, then Update — the
//      reference's order. A held-back packet whose real Check passes (possible only after an
//      earlier copy of it failed authentication) is opened right there, before the packets after it.
// Check only ever refuses more as updates accumulate, so the simulation (the real updates plus
// the ones for packets whose tag later fails) never lets through a packet the real window refuses
// unless another thread moved that window meanwhile. Statuses, window state and the lost /
// duplicate / out-of-window counters equal the sequential run; a refused packet's buffer is left
// untouched, as the reference leaves it, except in that concurrent case.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/nebula_aead.h"
#include "host_common.hpp"
#include "knobs.hpp"
#include "rxwin.hpp"
#include "relay.hpp"
#include "hip_guard.hpp"
#include "window_core.hpp"
#include "engine_internal.hpp"

using namespace neb_rx;

struct neb_window {
    WindowCore core;
    mutable std::mutex mu;  // ConnectionState.decryptLock (connection_state.go:100,112)
};

namespace {

struct RxProf {  // NEB_RX_PROF: the receives' phase times to stderr
    using T = std::chrono::steady_clock::time_point;
    static bool on() {
        static const bool v = std::getenv("NEB_RX_PROF") != nullptr;
        return v;
    }
    static T now() { return std::chrono::steady_clock::now(); }
    static double us(T a, T b) { return std::chrono::duration<double, std::micro>(b - a).count(); }
};

// every wire packet inside the arena (sums cannot wrap)
bool wire_in_arena(const neb_rx_packet* pk, uint32_t n, size_t arena_len) {
    for (uint32_t i = 0; i < n; i++)
        if (pk[i].off > arena_len || neb_rx_len(pk[i]) > arena_len - pk[i].off) return false;
    return true;
}

}  // namespace

extern "C" {

NEB_API int neb_window_create(uint64_t length, neb_window** out) {
    if (!out) return NEB_ERR_INVALID;
    *out = nullptr;
    if (length == 0 || (length & (length - 1))) return NEB_ERR_INVALID;  // NewBits panics (bits.go:29-31)
    neb_window* w = new (std::nothrow) neb_window;
    if (!w) return NEB_ERR_INVALID;
    w->core.length = length;
    w->core.mask = length - 1;
    w->core.words.assign(length >= 64 ? length / 64 : 1, 0);
    w->core.words[0] = 1;  // no counter 0: seeded as received (bits.go:47-48)
    *out = w;
    return NEB_OK;
}

NEB_API int neb_window_destroy(neb_window* w) {
    delete w;
    return NEB_OK;
}

NEB_API int neb_window_check(neb_window* w, uint64_t counter) {
    if (!w) return NEB_ERR_INVALID;
    std::lock_guard<std::mutex> g(w->mu);
    return w->core.check(counter) ? 1 : 0;
}

NEB_API int neb_window_update(neb_window* w, uint64_t counter) {
    if (!w) return NEB_ERR_INVALID;
    std::lock_guard<std::mutex> g(w->mu);
    return w->core.update(counter) ? 1 : 0;
}

NEB_API int neb_window_state(const neb_window* w, uint64_t* current, int64_t counters[3]) {
    if (!w) return NEB_ERR_INVALID;
    std::lock_guard<std::mutex> g(w->mu);
    if (current) *current = w->core.current;
    if (counters) {
        counters[0] = w->core.lost;
        counters[1] = w->core.dupe;
        counters[2] = w->core.out_of_window;
    }
    return NEB_OK;
}

NEB_API int neb_window_slot(const neb_window* w, uint64_t slot) {
    if (!w) return NEB_ERR_INVALID;
    std::lock_guard<std::mutex> g(w->mu);
    return w->core.get(slot) ? 1 : 0;
}

NEB_API int neb_window_reset_counters(neb_window* w) {
    if (!w) return NEB_ERR_INVALID;
    std::lock_guard<std::mutex> g(w->mu);
    w->core.lost = w->core.dupe = w->core.out_of_window = 0;
    return NEB_OK;
}

// Step 2 of neb_rx_open_batch_host: one GPU open for everything the simulation lets through (plan),
// compacted in arrival order into the engine's pinned staging (a zero-copy arena, opened on the
// receive stream) or a private vector (any other arena: neb_open_batch_host). verd[i]: admitted
// packet i's verdict; *ts, *td: the open's start and end.
static int open_admitted(neb_engine* e, int alg, const neb_desc* desc, uint32_t n, uint8_t* arena, size_t arena_len,
                         uint32_t key_hint, const uint8_t* plan, int32_t* verd, RxProf::T* ts, RxProf::T* td) {
    neb::RxStaging stage(e, alg, key_hint, arena, n);
    if (!stage.active() && stage.rc() != NEB_OK) return stage.rc();
    std::vector<uint32_t> sub_of(n);
    std::vector<neb_desc> sub;
    std::vector<int32_t> sub_status;
    const uint32_t ngpu = compact_admitted(desc, plan, n, sub_of.data(), [&](uint32_t m) {
        if (stage.active()) return stage.desc();
        sub.resize(m);
        sub_status.assign(m, NEB_STATUS_BAD_KEY);
        return sub.data();
    });
    int rc = NEB_OK;
    *ts = RxProf::now();
    if (ngpu)
        rc = stage.active() ? stage.open(ngpu)
                            : neb_open_batch_host(e, alg, sub.data(), ngpu, arena, arena_len, sub_status.data(), key_hint);
    *td = RxProf::now();
    // The verdicts are copied out of the staging statuses before the staging is released (on return):
    // they are the engine's shared pinned buffer, which the next receive call on this engine (another
    // thread) overwrites, or frees and reallocates for a larger batch, as soon as it holds rx.mu.
    const int32_t* gst = stage.active() ? stage.status() : sub_status.data();
    for (uint32_t i = 0; i < n && rc == NEB_OK; i++)
        if (plan[i]) verd[i] = gst[sub_of[i]];
    return rc;
}

NEB_API int neb_rx_open_batch_host(neb_engine* e, int alg, neb_window* const* windows, uint32_t nwindows,
                                   const neb_desc* desc, uint32_t n, uint8_t* arena, size_t arena_len,
                                   int32_t* status, uint32_t key_hint) {
    if (!e || (n && (!desc || !arena || !status || !windows))) return NEB_ERR_INVALID;
    if (n == 0) return NEB_OK;
    DeviceGuard dg;
    const auto now = RxProf::now;
    const auto t0 = now();
    RxPool& pool = rx_pool();
    auto with_window = [&](uint32_t g, auto&& fn) {
        std::lock_guard<std::mutex> lk(windows[g]->mu);
        fn(windows[g]->core);
    };
    auto par = [&](uint32_t cnt, auto&& fn) { pool.run(cnt, fn); };
    // an invalid batch is refused before any window moves or any packet is opened
    for (uint32_t i = 0; i < n; i++)
        if (!neb_desc_in_arena(desc[i], 1, arena_len)) return NEB_ERR_INVALID;
    const auto ta = now();
    const RxGroups G = group_by_window(
        n, nwindows, [&](uint32_t i) { return desc[i].key_id; }, [&](uint32_t g) { return windows[g] != nullptr; });
    const auto tb = now();
    const uint32_t nwg = window_group_count(G.start, nwindows, pool.size());
    const std::vector<uint32_t> wsplit = split_windows(G.start, nwindows, nwg);
    const auto tc = now();
    // 1. the simulation: opened[i] = 1 for the packets the sequential receive path would decrypt
    std::vector<uint8_t> opened = simulate_admits(G, wsplit, [&](uint32_t i) { return desc[i].counter; }, with_window, par);
    const auto t1 = now();
    // 2. one GPU open for them
    std::vector<int32_t> verd(n, NEB_STATUS_BAD_KEY);
    RxProf::T ts, td;
    int rc = open_admitted(e, alg, desc, n, arena, arena_len, key_hint, opened.data(), verd.data(), &ts, &td);
    if (rc != NEB_OK) return rc;
    const auto t2 = now();

    // 3. the real windows, each in arrival order: Check → tag verdict → Update (exact_rounds: a
    //    packet held back that its window accepts is opened with the rest of its window's run)
    for (uint32_t k = G.start[nwindows]; k < G.start[nwindows + 1]; k++) status[G.order[k]] = NEB_STATUS_BAD_KEY;
    // an extra round's open of packets pk through descriptors ds over arena ar; how: opened[]'s mark
    auto open_extra = [&](const std::vector<uint32_t>& pk, const neb_desc* ds, uint8_t* ar, size_t ar_len, uint8_t how) {
        std::vector<int32_t> st(pk.size(), NEB_STATUS_BAD_KEY);
        const int r = neb_open_batch_host(e, alg, ds, (uint32_t)pk.size(), ar, ar_len, st.data(), key_hint);
        for (size_t j = 0; j < pk.size() && r == NEB_OK; j++) {
            opened[pk[j]] = how;
            verd[pk[j]] = st[j];
        }
        return r;
    };
    // speculative verifications (exact_rounds' later rounds): each packet's AAD and ciphertext+tag
    // copied into a private arena and opened there; pt_at[i] = its plaintext's offset in it
    std::vector<uint8_t> spec;
    std::vector<uint64_t> pt_at;
    std::vector<uint32_t> commit, zero;
    rc = exact_rounds(
        window_runs(G, nwindows), nwg, [&](uint32_t k) { return desc[G.order[k]].counter; },
        [&](uint32_t k) { return G.order[k]; }, opened.data(), verd.data(), status, with_window,
        [&](const std::vector<uint32_t>& pk) -> int {
            std::vector<neb_desc> ds(pk.size());
            for (size_t j = 0; j < pk.size(); j++) ds[j] = desc[pk[j]];
            return open_extra(pk, ds.data(), arena, arena_len, 1);
        },
        [&](const std::vector<uint32_t>& pk) -> int {
            std::vector<neb_desc> ds(pk.size());
            std::vector<std::array<uint64_t, 3>> copies;
            pt_at.assign(n, 0);
            spec.clear();
            spec.resize(spec_layout(
                pk, [&](uint32_t i) -> const neb_desc& { return desc[i]; }, ds.data(), pt_at.data(),
                [&](uint64_t src, uint64_t dst, uint64_t len) { copies.push_back({src, dst, len}); }));
            for (const auto& c : copies) std::memcpy(spec.data() + c[1], arena + c[0], c[2]);
            return open_extra(pk, ds.data(), spec.data(), spec.size(), 2);
        },
        par, &commit, &zero);
    if (rc != NEB_OK) return rc;
    for (uint32_t i : commit) std::memcpy(arena + desc[i].dst_off, spec.data() + pt_at[i], desc[i].len);
    for (uint32_t i : zero) std::memset(arena + desc[i].dst_off, 0, desc[i].len);
    if (RxProf::on())
        std::fprintf(stderr,
                     "rx n=%u threads 1/%u plan %.1f us (validate %.1f group %.1f split %.1f sim %.1f) stage+gpu %.1f "
                     "(submit->done %.1f) real %.1f us\n",
                     n, nwg, RxProf::us(t0, t1), RxProf::us(t0, ta), RxProf::us(ta, tb), RxProf::us(tb, tc),
                     RxProf::us(tc, t1), RxProf::us(t1, t2), RxProf::us(ts, td), RxProf::us(t2, now()));
    return NEB_OK;
}

// ---- replay windows in device memory (rxwin.hip) ----------------------------------------------

}  // extern "C"

struct neb_dwindows {
    neb_engine* e = nullptr;
    neb::RxDevWin win{};
    neb::DevBuf<> mem;
    std::mutex mu;  // one receive batch at a time on a window set
    // ws_mem and wire_mem need no event (workspace.hpp): the receive ends every batch with its stream
    // synchronized, so nothing is in flight in them when the next batch, on any stream, takes d->mu
    neb::DevBuf<> ws_mem;
    neb::RxDevWs ws{};
    uint32_t ws_n = 0;
    neb::MappedBuf<uint32_t> h_host;  // 2 words (RxDevWs::need_host): a window needs the host; the scan failed
    // neb_rx_open_wire_batch: descriptors + gate statuses; then neb_rx_open_via_batch's compaction
    // (WireMem below): arrival indices, compacted statuses, per-workgroup counts, two counter words
    neb::DevBuf<> wire_mem;
    uint32_t wire_n = 0;
    uint32_t spin_limit = neb::kRxSpinLimit;  // neb_dwindows_set_spin_limit
    SchedSpacePtr sched;  // mixed-key AES-GCM receives: the open's scheduler workspace (rxwin.hpp RxBin)
    // neb_relay_forward_batch: the forward half's workspace (relay.hpp), which runs on after the
    // call returns, and one pinned word for the single target tunnel's key
    neb::HipWorkspace<> relay;
    neb::RelayWs relay_ws{};
    uint32_t relay_n = 0, relay_tun = 0;
    neb::PinnedBuf<uint32_t> relay_key;
    // neb_rx_open_via_batch: one pinned, mapped word, the unwrap kernel's count of inner packets
    neb::MappedBuf<uint32_t> via_count;
};

namespace {

#define RX_HIP(x)                               \
    do {                                        \
        if ((x) != hipSuccess) return NEB_ERR_HIP; \
    } while (0)

// Device slot w <-> a WindowCore (same length and word packing)
int dw_read(const neb_dwindows* d, uint32_t w, WindowCore& c) {
    const auto& v = d->win;
    c.length = v.length;
    c.mask = v.length - 1;
    c.words.resize(v.words);
    RX_HIP(hipMemcpy(&c.current, v.cur + w, 8, hipMemcpyDeviceToHost));
    RX_HIP(hipMemcpy(&c.lost, v.lost + w, 8, hipMemcpyDeviceToHost));
    RX_HIP(hipMemcpy(&c.dupe, v.dupe + w, 8, hipMemcpyDeviceToHost));
    RX_HIP(hipMemcpy(&c.out_of_window, v.oow + w, 8, hipMemcpyDeviceToHost));
    RX_HIP(hipMemcpy(c.words.data(), v.bits + (size_t)w * v.words, (size_t)v.words * 8, hipMemcpyDeviceToHost));
    return NEB_OK;
}
int dw_write(neb_dwindows* d, uint32_t w, const WindowCore& c) {
    const auto& v = d->win;
    const uint32_t one = 1;
    RX_HIP(hipMemcpy(v.cur + w, &c.current, 8, hipMemcpyHostToDevice));
    RX_HIP(hipMemcpy(v.lost + w, &c.lost, 8, hipMemcpyHostToDevice));
    RX_HIP(hipMemcpy(v.dupe + w, &c.dupe, 8, hipMemcpyHostToDevice));
    RX_HIP(hipMemcpy(v.oow + w, &c.out_of_window, 8, hipMemcpyHostToDevice));
    RX_HIP(hipMemcpy(v.bits + (size_t)w * v.words, c.words.data(), (size_t)v.words * 8, hipMemcpyHostToDevice));
    RX_HIP(hipMemcpy(v.present + w, &one, 4, hipMemcpyHostToDevice));
    // null-stream copies: complete before a non-blocking stream's batch reads the slot
    RX_HIP(hipStreamSynchronize(nullptr));
    return NEB_OK;
}

template <class T>
int d2h(std::vector<T>& h, const T* d, size_t n, hipStream_t s) {
    h.resize(n);
    if (n) RX_HIP(hipMemcpyAsync(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost, s));
    return NEB_OK;
}

}  // namespace

extern "C" {

NEB_API int neb_dwindows_create(neb_engine* e, uint32_t count, uint64_t length, neb_dwindows** out) {
    if (!e || !out || count == 0 || length == 0 || (length & (length - 1)) || length > (1ull << 24))
        return NEB_ERR_INVALID;
    *out = nullptr;
    DeviceGuard dg(neb_engine_device_of(e));
    std::unique_ptr<neb_dwindows> d(new (std::nothrow) neb_dwindows);
    if (!d) return NEB_ERR_INVALID;
    d->e = e;
    auto& v = d->win;
    v.count = count;
    v.length = length;
    v.words = length >= 64 ? (uint32_t)(length / 64) : 1u;
    v.words_lg = 0;
    while ((1u << v.words_lg) < v.words) v.words_lg++;
    const size_t b_present = neb::rx_align((size_t)count * 4), b_word = neb::rx_align((size_t)count * 8);
    const size_t bytes = b_present + 4 * b_word + (size_t)count * v.words * 8;
    RX_HIP(d->mem.reserve(bytes));
    RX_HIP(hipMemset(d->mem, 0, bytes));
    RX_HIP(hipStreamSynchronize(nullptr));
    RX_HIP(d->h_host.reserve(2 * sizeof(uint32_t)));
    uint8_t* m = d->mem;
    auto take = [&m](size_t b) { return (m += b) - b; };  // the next b bytes
    v.present = (uint32_t*)take(b_present);
    v.cur = (uint64_t*)take(b_word);
    v.lost = (int64_t*)take(b_word);
    v.dupe = (int64_t*)take(b_word);
    v.oow = (int64_t*)take(b_word);
    v.bits = (uint64_t*)m;
    *out = d.release();
    return NEB_OK;
}

NEB_API int neb_dwindows_destroy(neb_dwindows* d) {
    if (!d) return NEB_ERR_INVALID;
    DeviceGuard dg(neb_engine_device_of(d->e));
    {
        // neb_rx_open_batch returns only once its stream has run the batch, and holds d->mu
        // throughout: with the lock taken, nothing of this window set is in flight
        std::lock_guard<std::mutex> g(d->mu);
        d->relay.destroy();  // (waits: the forward half of the last relay batch may still be running)
    }
    delete d;  // with the engine's device current: the members release themselves (hip_owned.hpp)
    return NEB_OK;
}

NEB_API int neb_dwindows_load(neb_dwindows* d, uint32_t idx, const neb_window* w) {
    if (!d || idx >= d->win.count) return NEB_ERR_INVALID;
    std::lock_guard<std::mutex> g(d->mu);
    DeviceGuard dg(neb_engine_device_of(d->e));
    if (!w) {
        const uint32_t zero = 0;
        RX_HIP(hipMemcpy(d->win.present + idx, &zero, 4, hipMemcpyHostToDevice));
        RX_HIP(hipStreamSynchronize(nullptr));
        return NEB_OK;
    }
    WindowCore c;
    {
        std::lock_guard<std::mutex> lk(w->mu);
        c = w->core;
    }
    if (c.length != d->win.length) return NEB_ERR_INVALID;
    return dw_write(d, idx, c);
}

NEB_API int neb_dwindows_set_spin_limit(neb_dwindows* d, uint32_t limit) {
    if (!d) return NEB_ERR_INVALID;
    std::lock_guard<std::mutex> g(d->mu);
    d->spin_limit = limit;
    return NEB_OK;
}

NEB_API int neb_dwindows_store(neb_dwindows* d, uint32_t idx, neb_window* w) {
    if (!d || !w || idx >= d->win.count) return NEB_ERR_INVALID;
    std::lock_guard<std::mutex> g(d->mu);
    DeviceGuard dg(neb_engine_device_of(d->e));
    uint32_t present = 0;
    RX_HIP(hipMemcpy(&present, d->win.present + idx, 4, hipMemcpyDeviceToHost));
    if (!present) return NEB_ERR_INVALID;
    WindowCore c;
    const int rc = dw_read(d, idx, c);
    if (rc != NEB_OK) return rc;
    std::lock_guard<std::mutex> lk(w->mu);
    if (w->core.length != c.length) return NEB_ERR_INVALID;
    w->core = c;
    return NEB_OK;
}

}  // extern "C"

// The sequential finish of a device receive, for the windows the parallel one left (a tag failed, a
// counter near its wrap, the spin limit hit; rare): exact_rounds replays their packets in arrival order
// on host copies of the windows, opening in further device batches what it held back. d->mu held.
static int rx_host_finish(neb_engine* e, int alg, neb_dwindows* d, const neb_desc* d_desc, uint32_t n,
                          uint8_t* d_arena, int32_t* d_status, uint32_t key_hint, hipStream_t s) {
    int rc = NEB_OK;
    const auto& v = d->win;
    const neb::RxDevWs& ws = d->ws;
    std::vector<uint32_t> flag;
    if (d2h(flag, ws.wflag, v.count, s) != NEB_OK) return NEB_ERR_HIP;
    RX_HIP(hipStreamSynchronize(s));
    std::vector<uint32_t> run_w, run_i;
    std::vector<uint64_t> run_c;
    std::vector<uint8_t> adm;
    // windows' packet runs in run order (sorted by window: the runs are contiguous)
    auto runs_of = [&](const std::vector<uint32_t>& ws_list, auto&& fn) -> int {
        size_t k = 0;
        for (uint32_t w : ws_list) {
            while (k < n && run_w[k] < w) k++;
            const size_t k0 = k;
            while (k < n && run_w[k] == w) k++;
            const int r = fn(w, k0, k);
            if (r != NEB_OK) return r;
        }
        return NEB_OK;
    };
    std::vector<uint32_t> slow;
    for (uint32_t w = 0; w < v.count; w++)
        if ((flag[w] & neb::kRxTouched) && (flag[w] & (neb::kRxRisky | neb::kRxSlow))) slow.push_back(w);
    if (slow.empty()) return NEB_OK;
    // test hook: NEB_RXDEV_STRICT=1 refuses the host finish, to prove a batch ran the parallel form
    if (neb::knob(NEB_KNOB_RX_STRICT)) return NEB_ERR_INVALID;
    std::vector<int32_t> verdict, status;
    if (d2h(run_w, ws.run_w, n, s) || d2h(run_i, ws.run_i, n, s) || d2h(run_c, ws.run_c, n, s) ||
        d2h(adm, ws.adm, n, s) || d2h(verdict, ws.verdict, n, s) || d2h(status, d_status, n, s))
        return NEB_ERR_HIP;
    RX_HIP(hipStreamSynchronize(s));
    std::vector<ExactRun> runs;
    std::vector<WindowCore> cores(slow.size());
    std::vector<uint32_t> core_of(v.count, 0);
    rc = runs_of(slow, [&](uint32_t w, size_t k0, size_t k1) -> int {
        core_of[w] = (uint32_t)runs.size();
        runs.push_back({w, (uint32_t)k0, (uint32_t)k1});
        return dw_read(d, w, cores[core_of[w]]);
    });
    if (rc != NEB_OK) return rc;
    // speculative verifications: packets copied into a device scratch arena and opened there
    neb::DevBuf<> d_spec;
    std::vector<neb_desc> h_desc(n);
    std::vector<uint64_t> pt_at;
    std::vector<uint32_t> commit, zero;
    RX_HIP(hipMemcpyAsync(h_desc.data(), d_desc, (size_t)n * sizeof(neb_desc), hipMemcpyDeviceToHost, s));
    RX_HIP(hipStreamSynchronize(s));
    auto run_spans = [&](const uint8_t* src, uint8_t* dst, const std::vector<neb_span>& sp) -> int {
        if (sp.empty()) return NEB_OK;
        neb::DevBuf<neb_span> d_sp;
        RX_HIP(d_sp.reserve(sp.size() * sizeof(neb_span)));
        hipError_t err = hipMemcpyAsync(d_sp, sp.data(), sp.size() * sizeof(neb_span), hipMemcpyHostToDevice, s);
        if (err == hipSuccess) err = neb_rxdev_spans(src, dst, d_sp, (uint32_t)sp.size(), s);
        if (err == hipSuccess) err = hipStreamSynchronize(s);
        return err == hipSuccess ? NEB_OK : NEB_ERR_HIP;
    };
    rc = exact_rounds(
        runs, 1, [&](uint32_t k) { return run_c[k]; }, [&](uint32_t k) { return run_i[k]; }, adm.data(),
        verdict.data(), status.data(), [&](uint32_t w, auto&& fn) { fn(cores[core_of[w]]); },
        [&](const std::vector<uint32_t>& pk) -> int {  // one device open of these packets, in place
            const uint32_t cnt = (uint32_t)pk.size();
            RX_HIP(hipMemcpyAsync(ws.sub_map, pk.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, s));
            RX_HIP(hipMemcpyAsync(ws.nsub, &cnt, 4, hipMemcpyHostToDevice, s));
            RX_HIP(neb_rxdev_gather(d_desc, cnt, &ws, s));
            const int r = neb_launch(e, {.alg = alg, .open = 1, .desc = ws.sub_desc, .n = cnt, .arena = d_arena,
                                         .status = ws.sub_status, .key_hint = key_hint, .stream = s});
            if (r != NEB_OK) return r;
            std::vector<int32_t> st(cnt);
            RX_HIP(hipMemcpyAsync(st.data(), ws.sub_status, (size_t)cnt * 4, hipMemcpyDeviceToHost, s));
            RX_HIP(hipStreamSynchronize(s));
            for (uint32_t j = 0; j < cnt; j++) {
                adm[pk[j]] = 1;
                verdict[pk[j]] = st[j];
            }
            return NEB_OK;
        },
        [&](const std::vector<uint32_t>& pk) -> int {  // out of place, into a scratch arena
            const uint32_t cnt = (uint32_t)pk.size();
            std::vector<neb_span> sp;
            std::vector<neb_desc> ds(cnt);
            pt_at.assign(n, 0);
            const uint64_t bytes = spec_layout(
                pk, [&](uint32_t i) -> const neb_desc& { return h_desc[i]; }, ds.data(), pt_at.data(),
                [&](uint64_t src, uint64_t dst, uint64_t len) { sp.push_back({src, dst, (uint32_t)len, 0}); });
            d_spec.reset();  // (every round ends with s synchronized)
            RX_HIP(d_spec.reserve(bytes));
            int r = run_spans(d_arena, d_spec, sp);
            if (r != NEB_OK) return r;
            neb::DevBuf<neb_desc> d_ds;
            neb::DevBuf<int32_t> d_st;
            RX_HIP(d_ds.reserve((size_t)cnt * sizeof(neb_desc)));
            RX_HIP(d_st.reserve((size_t)cnt * 4));
            std::vector<int32_t> st(cnt, NEB_STATUS_BAD_KEY);
            hipError_t err = hipMemcpyAsync(d_ds, ds.data(), (size_t)cnt * sizeof(neb_desc), hipMemcpyHostToDevice, s);
            r = err != hipSuccess ? NEB_ERR_HIP
                                  : neb_launch(e, {.alg = alg, .open = 1, .desc = d_ds, .n = cnt, .arena = d_spec,
                                                   .status = d_st, .key_hint = key_hint, .stream = s});
            if (r == NEB_OK && (hipMemcpyAsync(st.data(), d_st, (size_t)cnt * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                                hipStreamSynchronize(s) != hipSuccess))
                r = NEB_ERR_HIP;
            if (r != NEB_OK) return r;
            for (uint32_t j = 0; j < cnt; j++) {
                adm[pk[j]] = 2;
                verdict[pk[j]] = st[j];
            }
            return NEB_OK;
        },
        [](uint32_t cnt, auto&& fn) {
            for (uint32_t j = 0; j < cnt; j++) fn(j);
        },
        &commit, &zero);
    if (rc == NEB_OK && (!commit.empty() || !zero.empty())) {
        std::vector<neb_span> back, zsp;
        for (uint32_t i : commit) back.push_back({pt_at[i], h_desc[i].dst_off, h_desc[i].len, 0});
        for (uint32_t i : zero) zsp.push_back({0, h_desc[i].dst_off, h_desc[i].len, 0});
        rc = run_spans(d_spec, d_arena, back);
        if (rc == NEB_OK) rc = run_spans(nullptr, d_arena, zsp);
    }
    if (rc != NEB_OK) return rc;
    for (size_t r = 0; r < runs.size(); r++)
        if ((rc = dw_write(d, runs[r].w, cores[r])) != NEB_OK) return rc;
    RX_HIP(hipMemcpyAsync(d_status, status.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
    RX_HIP(hipStreamSynchronize(s));
    return NEB_OK;
}

// neb_rx_open_batch with d->mu held (the wire form builds its descriptors under the same lock)
static int rx_open_batch_locked(neb_engine* e, int alg, neb_dwindows* d, const neb_desc* d_desc, uint32_t n,
                                uint8_t* d_arena, int32_t* d_status, uint32_t key_hint, void* stream) {
    int rc = NEB_OK;
    hipSetDevice(neb_engine_device_of(e));
    hipStream_t s = (hipStream_t)stream;
    auto& v = d->win;
    if (n > d->ws_n) {
        d->ws_n = 0;
        RX_HIP(d->ws_mem.reserve(neb::rx_ws_layout(n, v.count, v.words, nullptr, nullptr), nullptr,
                                 [&] { return hipStreamSynchronize(s); }));
        neb::rx_ws_layout(n, v.count, v.words, d->ws_mem, &d->ws);

        // the scratch bitmap is zeroed once here and again by each batch as it is consumed
        RX_HIP(hipMemsetAsync(d->ws.scratch, 0, ((size_t)v.count << v.words_lg) * 8, s));
        RX_HIP(hipMemsetAsync(d->ws.mixed, 0, 4, s));  // no generation is 0
        d->ws.gen = UINT32_MAX;  // the first batch clears the first-occurrence table
        d->ws_n = n;
    }
    // a new generation per batch empties the first-occurrence table; cleared for real at wrap
    if (++d->ws.gen == 0) {  // (every generation-tagged word: the table, the block granules, wrisky)
        const size_t nblk = ((size_t)d->ws_n + neb::kRxBlock - 1) / neb::kRxBlock;
        RX_HIP(hipMemsetAsync(d->ws.tab_owner, 0, (size_t)8 << d->ws.tab_lg, s));
        RX_HIP(hipMemsetAsync(d->ws.tab_min, 0, (size_t)8 << d->ws.tab_lg, s));
        RX_HIP(hipMemsetAsync(d->ws.blk_pub, 0, nblk * 3 * 8, s));
        RX_HIP(hipMemsetAsync(d->ws.wrisky, 0, (size_t)v.count * 4, s));
        d->ws.gen = 1;
    }
    d->h_host[0] = d->h_host[1] = 0;
    d->ws.need_host = d->h_host;
    d->ws.spin_limit = d->spin_limit;
    const neb::RxDevWs& ws = d->ws;

    const auto now = RxProf::now;
    const auto us = RxProf::us;
    const auto t0 = now();
    // Everything is queued at once, one host read at the end: windows whose counters come within
    // 2^62 of wrapping hold all their packets back (admitted by none), and exact_rounds opens what
    // their real pass accepts in batches, like the windows where a tag failed.
    // 0. mixed-key AES-GCM: the open's binning (sched_body.hpp) reads only the descriptors, so extra
    //    workgroups of the plan's own launches run it (rxwin.hpp RxBin): three launches off the chain.
    //    A batch large enough for sub-bins is binned by the open itself.
    SchedSpace* prebinned = nullptr;
    neb::RxBin bin{};
    if (alg == NEB_ALG_AESGCM && key_hint == NEB_KEYS_MIXED && (int64_t)n < neb::knob(NEB_KNOB_SUB_BINS_FROM)) {
        if (!d->sched) d->sched.reset(neb_sched_space_new());
        if (!d->sched) return NEB_ERR_HIP;
        if ((rc = neb_rx_sched_begin(e, n, d->sched.get(), s, &bin.ws, &bin.max_keys)) != NEB_OK) return rc;
        bin.on = 1;
        prebinned = d->sched.get();
    }
    // 1. group by window, prefix maxima, first occurrences; admission for the safe windows
    if (neb_rxdev_plan(d_desc, n, &v, &ws, d_status, &bin, s) != hipSuccess) {
        if (prebinned) neb_rx_sched_abort(prebinned);
        return NEB_ERR_HIP;
    }
    const auto t1 = now();
    // 2. one open over the batch that runs the admitted packets only (the plan's mask), writing their
    //    statuses at their arrival indices
    rc = neb_launch(e, {.alg = alg, .open = 1, .desc = d_desc, .n = n, .arena = d_arena, .status = d_status,
                        .key_hint = key_hint, .stream = s, .sched = prebinned, .prebinned = prebinned != nullptr,
                        .rx = ws.adm});
    if (rc != NEB_OK) return rc;
    const auto t2 = now();
    // 3. the verdicts into the windows, and the parallel finish of every window whose packets all verified
    RX_HIP(neb_rxdev_finish(n, &v, &ws, d_status, s));
    const auto t3 = now();
    RX_HIP(hipStreamSynchronize(s));
    if (RxProf::on())
        std::fprintf(stderr, "rxdev n=%u enqueue plan %.1f, open %.1f, finish %.1f us, wait %.1f us\n", n, us(t0, t1),
                     us(t1, t2), us(t2, t3), us(t3, now()));
    // the plan and the open flag, in pinned host memory, whether any window needs the sequential finish
    const uint32_t need = __atomic_load_n(&d->h_host[0], __ATOMIC_ACQUIRE);
    if (__atomic_load_n(&d->h_host[1], __ATOMIC_ACQUIRE)) return NEB_ERR_HIP;  // a scan lookback timed out
    if (need == 0) return NEB_OK;
    return rx_host_finish(e, alg, d, d_desc, n, d_arena, d_status, key_hint, s);
}

// relayed: pk are the inner records of neb_rx_open_via_batch_host and status[] holds the unwrap's
// marks: a record marked NEB_STATUS_NOT_RELAYED keeps that status, the others pass the gate with
// relayed = true.
static int rx_open_wire_host(neb_engine* e, int alg, neb_window* const* windows, uint32_t nwindows,
                             const neb_rx_packet* pk, uint32_t n, uint8_t* arena, size_t arena_len, int32_t* status,
                             uint32_t key_hint, bool relayed) {
    if (!e || (n && (!pk || !arena || !status || !windows))) return NEB_ERR_INVALID;
    if (n == 0) return NEB_OK;
    if (!wire_in_arena(pk, n, arena_len)) return NEB_ERR_INVALID;
    std::vector<neb_desc> desc(n);
    std::vector<int32_t> gate(n);
    for (uint32_t i = 0; i < n; i++) {
        neb_desc dd{pk[i].off, pk[i].off, pk[i].off, 0, 0, 0, NEB_KEYS_MIXED, 0};
        gate[i] = relayed && status[i] == NEB_STATUS_NOT_RELAYED ? NEB_STATUS_NOT_RELAYED
                                                                 : neb_rx_wire_gate(arena + pk[i].off, pk[i], &dd, relayed);
        if (gate[i] != NEB_STATUS_OK) dd = neb_desc{pk[i].off, pk[i].off, pk[i].off, 0, 0, 0, NEB_KEYS_MIXED, 0};
        desc[i] = dd;
    }
    const int rc = neb_rx_open_batch_host(e, alg, windows, nwindows, desc.data(), n, arena, arena_len, status, key_hint);
    if (rc != NEB_OK) return rc;
    for (uint32_t i = 0; i < n; i++)
        if (gate[i] != NEB_STATUS_OK) status[i] = gate[i];
    return NEB_OK;
}

extern "C" {

NEB_API int neb_rx_open_batch(neb_engine* e, int alg, neb_dwindows* d, const neb_desc* d_desc, uint32_t n,
                              uint8_t* d_arena, int32_t* d_status, uint32_t key_hint, void* stream) {
    if (!e || !d || d->e != e || (n && (!d_desc || !d_arena || !d_status))) return NEB_ERR_INVALID;
    int rc = neb_check_batch_args(e, alg, key_hint);
    if (rc != NEB_OK) return rc;
    if (n == 0) return NEB_OK;
    DeviceGuard dg;
    std::lock_guard<std::mutex> g(d->mu);
    return rx_open_batch_locked(e, alg, d, d_desc, n, d_arena, d_status, key_hint, stream);
}

// readOutsidePackets' gate (neb_rx_wire_gate) on the host, then the batched receive over the
// descriptors it builds; refused packets carry an empty descriptor with no key (untouched by the
// receive) and get the gate's status.
NEB_API int neb_rx_open_wire_batch_host(neb_engine* e, int alg, neb_window* const* windows, uint32_t nwindows,
                                        const neb_rx_packet* pk, uint32_t n, uint8_t* arena, size_t arena_len,
                                        int32_t* status, uint32_t key_hint) {
    return rx_open_wire_host(e, alg, windows, nwindows, pk, n, arena, arena_len, status, key_hint, false);
}

}  // extern "C"

// d->wire_mem carved for a capacity of n packets: the wire receive's descriptors and gate statuses,
// then what neb_rx_open_via_batch's compacted phase 2 adds (the compacted batch's statuses and
// arrival indices, the unwrap kernel's per-workgroup counts and its two counter words)
struct WireMem {
    neb_desc* desc;
    int32_t *gate, *sub;
    uint32_t *map, *blk, *tot;
    static size_t bytes(uint32_t n) { return (size_t)n * (sizeof(neb_desc) + 12) + ((size_t)(n + 255u) / 256u + 2) * 4; }
    WireMem(uint8_t* m, uint32_t n) {
        desc = (neb_desc*)m;
        gate = (int32_t*)(desc + n);
        sub = gate + n;
        map = (uint32_t*)(sub + n);
        blk = map + n;
        tot = blk + ((size_t)n + 255u) / 256u;
    }
};
struct RxViaArgs {  // neb_rx_open_via_batch's arrays for the unwrap
    const neb_rx_via* d_via;
    neb_rx_packet* d_inner_pk;
    int32_t* d_inner_status;
};

// neb_rx_open_wire_batch with d->mu held and the engine's device current (the relay forwarding runs
// its forward half under the same lock). via: the unwrap of neb_rx_open_via_batch runs in place of
// the status fix (one kernel for both), and its count, in the pinned word d->via_count, arrives
// with the synchronize that ends the receive.
static int rx_open_wire_locked(neb_engine* e, int alg, neb_dwindows* d, const neb_rx_packet* d_pk, uint32_t n,
                               uint8_t* d_arena, int32_t* d_status, uint32_t key_hint, void* stream,
                               const RxViaArgs* via = nullptr) {
    int rc = NEB_OK;
    hipStream_t s = (hipStream_t)stream;
    if (n > d->wire_n) {
        d->wire_n = 0;
        RX_HIP(d->wire_mem.reserve(WireMem::bytes(n), nullptr, [&] { return hipStreamSynchronize(s); }));
        d->wire_n = n;
        RX_HIP(hipMemsetAsync(WireMem(d->wire_mem, n).tot, 0, 8, s));  // zero between batches from here on
    }
    const WireMem wm(d->wire_mem, d->wire_n);
    neb_desc* wd = wm.desc;
    int32_t* gate = wm.gate;
    RX_HIP(neb_rxdev_wire(d_pk, n, d_arena, wd, gate, s));
    rc = rx_open_batch_locked(e, alg, d, wd, n, d_arena, d_status, key_hint, stream);
    if (rc != NEB_OK) return rc;
    if (via)
        RX_HIP(neb_rxdev_via_unwrap(gate, d_status, d_pk, via->d_via, n, d_arena, via->d_inner_pk, via->d_inner_status,
                                    wm.blk, wm.tot, d->via_count, s));
    else
        RX_HIP(neb_rxdev_wire_fix(gate, d_status, n, s));
    RX_HIP(hipStreamSynchronize(s));
    return NEB_OK;
}

// The forward half's workspace, grown as the receive's is (no allocation in the steady state).
static int relay_reserve(neb_dwindows* d, uint32_t n, uint32_t ntun) {
    RX_HIP(d->relay_key.reserve(sizeof(uint32_t)));
    if (d->relay.mem() && n <= d->relay_n && ntun <= d->relay_tun) return NEB_OK;
    const uint32_t nc = std::max({n, d->relay_n, 1024u}), tc = std::max({ntun, d->relay_tun, 64u});
    size_t cub = 0;
    const size_t bytes = neb_relay_ws_bytes(nc, tc, &cub);
    d->relay_n = d->relay_tun = 0;
    RX_HIP(d->relay.reserve(bytes));  // (laid out again whether it grew or not: the capacities changed)
    neb::relay_ws_layout(nc, tc, cub, d->relay.mem(), &d->relay_ws);
    d->relay_n = nc;
    d->relay_tun = tc;
    return NEB_OK;
}

extern "C" {

NEB_API int neb_rx_open_wire_batch(neb_engine* e, int alg, neb_dwindows* d, const neb_rx_packet* d_pk, uint32_t n,
                                   uint8_t* d_arena, int32_t* d_status, uint32_t key_hint, void* stream) {
    if (!e || !d || d->e != e || (n && (!d_pk || !d_arena || !d_status))) return NEB_ERR_INVALID;
    int rc = neb_check_batch_args(e, alg, key_hint);
    if (rc != NEB_OK) return rc;
    if (n == 0) return NEB_OK;
    std::lock_guard<std::mutex> g(d->mu);
    DeviceGuard dg(neb_engine_device_of(e));
    return rx_open_wire_locked(e, alg, d, d_pk, n, d_arena, d_status, key_hint, stream);
}

// ---- relay forwarding: the receive, then SendVia in place (relay.hpp, relay.hip) -----------------

NEB_API int neb_relay_forward_batch(neb_engine* e, int alg, neb_dwindows* d, const neb_rx_packet* d_pk,
                                    const neb_relay_route* d_route, uint32_t n, neb_tx_tunnel* d_tunnels,
                                    uint32_t ntunnels, uint8_t* d_arena, int32_t* d_status, int32_t* d_fwd_status,
                                    uint32_t key_hint, void* stream) {
    if (!e || !d || d->e != e || (n && (!d_pk || !d_route || !d_arena || !d_status || !d_fwd_status)) ||
        (ntunnels && !d_tunnels))
        return NEB_ERR_INVALID;
    int rc = neb_check_batch_args(e, alg, key_hint);
    if (rc != NEB_OK) return rc;
    if (n == 0) return NEB_OK;
    std::lock_guard<std::mutex> g(d->mu);
    DeviceGuard dg(neb_engine_device_of(e));
    hipStream_t s = (hipStream_t)stream;
    if ((rc = relay_reserve(d, n, ntunnels)) != NEB_OK) return rc;
    RX_HIP(d->relay.begin(s));  // after the last batch's forward half, if that ran on another stream
    // one target tunnel: its key, for the single-key seal (read back while the receive runs, which
    // ends with the stream synchronized)
    *d->relay_key = NEB_KEYS_MIXED;
    if (ntunnels == 1)
        RX_HIP(hipMemcpyAsync(d->relay_key, &d_tunnels[0].key_id, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if ((rc = rx_open_wire_locked(e, alg, d, d_pk, n, d_arena, d_status, key_hint, stream)) != NEB_OK) return rc;
    const uint32_t seal_hint = ntunnels == 1 && neb_key_alg(e, *d->relay_key) == alg ? *d->relay_key : NEB_KEYS_MIXED;
    const uint32_t* d_keys = nullptr;
    uint32_t max_keys = 0;
    neb_engine_key_table(e, &d_keys, &max_keys);
    const neb::RelayWs& ws = d->relay_ws;
    RX_HIP(neb_relay_plan(d_pk, d_route, d_status, n, d_tunnels, ntunnels, d_keys, max_keys, alg, d_arena, d_fwd_status,
                          &ws, s));
    rc = neb_launch(e, {.alg = alg, .open = 0, .desc = ws.sub_desc, .n = n, .d_n = ws.nsub, .arena = d_arena,
                        .status = ws.sub_status, .key_hint = seal_hint, .stream = s, .note_use = true});
    if (rc == NEB_OK && neb_relay_fix(&ws, n, d_fwd_status, s) != hipSuccess) rc = NEB_ERR_HIP;
    (void)d->relay.end(s);
    return rc;
}

// The host form: the receive over the host arena, then the same per-packet rules (neb_relay_gate,
// neb_relay_send_via) as a plain loop in arrival order, and one seal batch over the forwarded packets.
NEB_API int neb_relay_forward_batch_host(neb_engine* e, int alg, neb_window* const* windows, uint32_t nwindows,
                                         const neb_rx_packet* pk, const neb_relay_route* route, uint32_t n,
                                         neb_tx_tunnel* tunnels, uint32_t ntunnels, uint8_t* arena, size_t arena_len,
                                         int32_t* status, int32_t* fwd_status, uint32_t key_hint) {
    if (!e || (n && (!route || !fwd_status)) || (ntunnels && !tunnels)) return NEB_ERR_INVALID;
    int rc = neb_rx_open_wire_batch_host(e, alg, windows, nwindows, pk, n, arena, arena_len, status, key_hint);
    if (rc != NEB_OK || n == 0) return rc;
    std::vector<neb_desc> desc;
    std::vector<uint32_t> map;
    for (uint32_t i = 0; i < n; i++) {
        uint8_t* p = arena + pk[i].off;
        int32_t st = neb_relay_gate(status[i], p, route[i], tunnels, ntunnels,
                                    [&](uint32_t key) { return neb_key_alg(e, key) == alg; });
        if (st == NEB_STATUS_OK) {
            neb_tx_tunnel& t = tunnels[route[i].tunnel];
            uint32_t hdr[4];
            neb_desc dd;
            st = neb_relay_send_via(pk[i], route[i].remote_index, t.key_id, ++t.message_counter, hdr, &dd);
            if (st == NEB_STATUS_OK) {
                std::memcpy(p, hdr, 16);
                desc.push_back(dd);
                map.push_back(i);
            }
        }
        fwd_status[i] = st;
    }
    if (desc.empty()) return NEB_OK;
    std::vector<int32_t> sub(desc.size(), NEB_STATUS_OK);
    const uint32_t seal_hint = ntunnels == 1 ? tunnels[0].key_id : NEB_KEYS_MIXED;
    rc = neb_seal_batch_host(e, alg, desc.data(), (uint32_t)desc.size(), arena, arena_len, sub.data(), seal_hint);
    if (rc != NEB_OK) return rc;
    for (size_t j = 0; j < sub.size(); j++)
        if (sub[j] != NEB_STATUS_OK) fwd_status[map[j]] = sub[j];
    return NEB_OK;
}

}  // extern "C"

// ---- receive through a relay: VerifyRelay, then unwrap and open (rxwin.hpp neb_rx_via_unwrap) -----

extern "C" {

NEB_API int neb_rx_via_unwrap_host(const neb_rx_packet* pk, const neb_rx_via* via, const int32_t* status, uint32_t n,
                                   const uint8_t* arena, size_t arena_len, neb_rx_packet* inner_pk,
                                   int32_t* inner_status) {
    if (n && (!pk || !via || !status || !arena || !inner_pk || !inner_status)) return NEB_ERR_INVALID;
    if (!wire_in_arena(pk, n, arena_len)) return NEB_ERR_INVALID;
    for (uint32_t i = 0; i < n; i++) {
        const bool ok = status[i] == NEB_STATUS_OK && neb_rx_len(pk[i]) >= 2u;
        const uint8_t* h = arena + pk[i].off;
        const bool el = neb_rx_via_unwrap(status[i], ok ? h[0] : 0, ok ? h[1] : 0, pk[i], via[i], &inner_pk[i]);
        inner_status[i] = el ? NEB_STATUS_OK : NEB_STATUS_NOT_RELAYED;
    }
    return NEB_OK;
}

NEB_API int neb_rx_open_via_batch_host(neb_engine* e, int alg, neb_window* const* windows, uint32_t nwindows,
                                       const neb_rx_packet* pk, const neb_rx_via* via, uint32_t n, uint8_t* arena,
                                       size_t arena_len, int32_t* status, neb_rx_packet* inner_pk,
                                       int32_t* inner_status, uint32_t key_hint, uint32_t inner_key_hint) {
    if (!e || (n && (!via || !inner_pk || !inner_status))) return NEB_ERR_INVALID;
    int rc = neb_rx_open_wire_batch_host(e, alg, windows, nwindows, pk, n, arena, arena_len, status, key_hint);
    if (rc != NEB_OK || n == 0) return rc;
    if ((rc = neb_rx_via_unwrap_host(pk, via, status, n, arena, arena_len, inner_pk, inner_status)) != NEB_OK) return rc;
    bool any = false;
    for (uint32_t i = 0; i < n && !any; i++) any = inner_status[i] != NEB_STATUS_NOT_RELAYED;
    if (!any) return NEB_OK;
    return rx_open_wire_host(e, alg, windows, nwindows, inner_pk, n, arena, arena_len, inner_status, inner_key_hint, true);
}

NEB_API int neb_rx_open_via_batch(neb_engine* e, int alg, neb_dwindows* d, const neb_rx_packet* d_pk,
                                  const neb_rx_via* d_via, uint32_t n, uint8_t* d_arena, int32_t* d_status,
                                  neb_rx_packet* d_inner_pk, int32_t* d_inner_status, uint32_t key_hint,
                                  uint32_t inner_key_hint, void* stream) {
    if (!e || !d || d->e != e || (n && (!d_pk || !d_via || !d_arena || !d_status || !d_inner_pk || !d_inner_status)))
        return NEB_ERR_INVALID;
    int rc = neb_check_batch_args(e, alg, key_hint);
    if (rc == NEB_OK) rc = neb_check_batch_args(e, alg, inner_key_hint);
    if (rc != NEB_OK) return rc;
    if (n == 0) return NEB_OK;
    std::lock_guard<std::mutex> g(d->mu);
    DeviceGuard dg(neb_engine_device_of(e));
    hipStream_t s = (hipStream_t)stream;
    RX_HIP(d->via_count.reserve(sizeof(uint32_t)));
    *d->via_count = 0;
    const RxViaArgs via{d_via, d_inner_pk, d_inner_status};
    if ((rc = rx_open_wire_locked(e, alg, d, d_pk, n, d_arena, d_status, key_hint, stream, &via)) != NEB_OK) return rc;
    // no terminal relay packet verified: every inner_status is NEB_STATUS_NOT_RELAYED already
    const uint32_t m = __atomic_load_n(&d->via_count[0], __ATOMIC_ACQUIRE);
    if (m == 0) return NEB_OK;
    if (m > n) return NEB_ERR_HIP;
    // phase 2 over the m inner packets, compacted in arrival order; phase 1 is done with wire_mem
    const WireMem wm(d->wire_mem, d->wire_n);
    RX_HIP(neb_rxdev_wire_inner(d_inner_pk, d_inner_status, n, d_arena, wm.blk, m, wm.desc, wm.gate, wm.map, s));
    if ((rc = rx_open_batch_locked(e, alg, d, wm.desc, m, d_arena, wm.sub, inner_key_hint, stream)) != NEB_OK) return rc;
    RX_HIP(neb_rxdev_via_fix(wm.gate, wm.sub, wm.map, m, d_inner_status, s));
    RX_HIP(hipStreamSynchronize(s));
    return NEB_OK;
}

}  // extern "C"
