// conntrack_core.hpp — the rules of the connection table (neb_conntrack_*), shared by the host-only
// table and the host forms (conntrack.cpp), the device form (conntrack.hip) and the sanitizer program
// (tests/sanitize_conntrack). Plain C++17; compiles with g++ alone (no HIP headers).
//
// Restated from slackhq/nebula (read as text, not copied):
//   firewall.Packet, the map's key          firewall.go:30-38 (firewall/packet.go)
//   inConns                                 firewall.go:505-576
//   addConn                                 firewall.go:578-601
//   evict                                   firewall.go:603-630
//
// Every step takes a memory policy M with load, store, cas (returns the word it found), fetch_max,
// fetch_add and fetch_sub over one 64-bit word: the device binds them to 8-byte agent-scope atomics,
// the host to __atomic builtins, so the host forms may run beside each other as the device launches do.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/nebula_aead.h"

#ifndef NEB_RT_HD
#if defined(__HIPCC__)
#define NEB_RT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define NEB_RT_HD inline
#endif
#endif

namespace neb {

// One slot of the open-addressing table: linear probing over a power-of-two number of slots, at least
// 2 x capacity, one 64-byte line each. Within one image a slot only moves EMPTY -> CLAIMED -> SETTLED
// -> TOMB (an add's two launches, then an evict); tombstones are not reused, a compaction into a
// cleared image drops them, so the words of an EMPTY slot are always zero.
struct alignas(64) CtSlot {
    uint64_t state;    // kCtEmpty, kCtTomb, ct_claimed(owner, fp) or ct_settled(fp)
    uint64_t key[5];   // CtKey, written by the claiming add before the state says SETTLED
    uint64_t expires;  // conn.Expires, ns of the caller's monotonic clock
    uint64_t meta;     // rulesVersion << 1 | incoming; during an add: | (batch index + 1) << 32
};
static_assert(sizeof(CtSlot) == 64, "one slot, one line");

constexpr uint64_t kCtEmpty = 0, kCtTomb = 1;
constexpr uint64_t kCtKindMask = 3ull << 62, kCtClaimed = 2ull << 62, kCtSettled = 3ull << 62;
constexpr uint32_t kCtMaxCapacity = 1u << 22;
constexpr uint32_t kCtNoSlot = 0xFFFFFFFFu;

// The owner is an index into the batch that claims (an add's keys, or the old image's slots: below
// 2^23 either way).
NEB_RT_HD uint64_t ct_claimed(uint32_t owner, uint32_t fp) { return kCtClaimed | ((uint64_t)owner << 32) | fp; }
NEB_RT_HD uint64_t ct_settled(uint32_t fp) { return kCtSettled | fp; }
NEB_RT_HD uint32_t ct_state_owner(uint64_t s) { return (uint32_t)(s >> 32) & 0x3FFFFFFFu; }
NEB_RT_HD uint32_t ct_state_fp(uint64_t s) { return (uint32_t)s; }
NEB_RT_HD uint64_t ct_meta(uint32_t version, uint32_t incoming) { return ((uint64_t)(version & 0xFFFFu) << 1) | (incoming ? 1u : 0u); }
// The copy with the highest batch index wins the slot's atomic max, as sequential addConn calls
// would leave it; index + 1, so that every copy beats the settled word of an entry that exists.
NEB_RT_HD uint64_t ct_meta_in_add(uint32_t index, uint32_t version, uint32_t incoming) {
    return ((uint64_t)(index + 1u) << 32) | ct_meta(version, incoming);
}

NEB_RT_HD uint32_t ct_slots_for(uint32_t capacity) {  // capacity <= 2^22
    uint32_t s = 2;
    while (s < 2u * capacity) s <<= 1;
    return s;
}

// firewall.Packet as five words. The address words are the bytes as little-endian integers; for
// family 4 only the first four count (the input's bytes 4..15 are not trusted), so a 4-in-6 address
// (family 6) never equals its IPv4 form.
struct CtKey {
    uint64_t w[5];
};
NEB_RT_HD bool ct_key_eq(const CtKey& a, const CtKey& b) {
    return ((a.w[0] ^ b.w[0]) | (a.w[1] ^ b.w[1]) | (a.w[2] ^ b.w[2]) | (a.w[3] ^ b.w[3]) | (a.w[4] ^ b.w[4])) == 0;
}
// q: the 48 bytes of a neb_fw_packet as six little-endian 64-bit words.
NEB_RT_HD CtKey ct_key_from_words(const uint64_t q[6]) {
    const uint32_t family = (uint32_t)(q[4] >> 40) & 0xFFu, flags = (uint32_t)(q[4] >> 48) & 0xFFu;
    const bool v4 = family == 4u;
    CtKey k;
    k.w[0] = v4 ? (q[0] & 0xFFFFFFFFull) : q[0];
    k.w[1] = v4 ? 0 : q[1];
    k.w[2] = v4 ? (q[2] & 0xFFFFFFFFull) : q[2];
    k.w[3] = v4 ? 0 : q[3];
    // local_port | remote_port << 16 | protocol << 32 | family << 40 | Fragment << 48
    k.w[4] = (q[4] & 0xFFFFFFFFFFFFull) | ((uint64_t)(flags & NEB_FW_FRAGMENT) << 48);
    return k;
}
NEB_RT_HD uint32_t ct_key_protocol(const CtKey& k) { return (uint32_t)(k.w[4] >> 32) & 0xFFu; }

// The keyed hash: the table's seed goes in first, so which 5-tuples share a chain is not known to a
// peer. The low bits pick the home slot, the high 32 are the fingerprint kept in the state word.
NEB_RT_HD uint64_t ct_mix(uint64_t h) {
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    return h ^ (h >> 32);
}
NEB_RT_HD uint64_t ct_hash(uint64_t seed, const CtKey& k) {
    uint64_t h = ct_mix(seed ^ 0x9E3779B97F4A7C15ull);
    for (int i = 0; i < 5; i++) h = ct_mix(h ^ k.w[i]) + 0x9E3779B97F4A7C15ull;
    return ct_mix(h ^ seed);
}
NEB_RT_HD uint32_t ct_home(uint64_t h, uint32_t mask) { return (uint32_t)h & mask; }
NEB_RT_HD uint32_t ct_fp(uint64_t h) { return (uint32_t)(h >> 32); }

// What a table is made with, and what changes between calls.
struct CtParams {
    uint64_t seed;
    uint64_t tcp_ns, udp_ns, default_ns;  // firewall.go:562-569
    uint32_t mask;                        // slots - 1
    uint32_t capacity;
};
NEB_RT_HD uint64_t ct_timeout(const CtParams& p, uint32_t protocol) {
    return protocol == 6u ? p.tcp_ns : protocol == 17u ? p.udp_ns : p.default_ns;
}

template <class M>
NEB_RT_HD CtKey ct_slot_key(const CtSlot* s, M m) {
    CtKey k;
    for (int i = 0; i < 5; i++) k.w[i] = m.load(&s->key[i]);
    return k;
}

// The search of a settled key: from its home slot to the key or to the first EMPTY slot. A CLAIMED
// slot belongs to an add whose second launch has not run: not this key yet, go on (the miss
// linearises before the add). The table always keeps EMPTY slots; the bound only guards an image
// whose tombstones have filled it.
template <class M>
NEB_RT_HD bool ct_find(CtSlot* slots, const CtParams& p, const CtKey& k, uint64_t h, M m, uint32_t* slot) {
    const uint64_t want = ct_settled(ct_fp(h));
    uint32_t s = ct_home(h, p.mask);
    for (uint32_t n = 0; n <= p.mask; n++, s = (s + 1u) & p.mask) {
        const uint64_t st = m.load(&slots[s].state);
        if (st == kCtEmpty) return false;
        if (st == want && ct_key_eq(ct_slot_key(&slots[s], m), k)) {
            *slot = s;
            return true;
        }
    }
    return false;
}

// ---- lookup (inConns) ---------------------------------------------------------------------------

// The verdict byte: NEB_CT_* | NEB_CT_INCOMING for a STALE entry that was added as incoming.
template <class M>
NEB_RT_HD uint32_t ct_lookup_one(CtSlot* slots, const CtParams& p, uint32_t version, uint64_t now, const CtKey& k, M m) {
    uint32_t s;
    if (!ct_find(slots, p, k, ct_hash(p.seed, k), m, &s)) return NEB_CT_MISS;
    const uint32_t meta = (uint32_t)m.load(&slots[s].meta);
    if (((meta >> 1) & 0xFFFFu) != (version & 0xFFFFu)) return NEB_CT_STALE | ((meta & 1u) ? (uint32_t)NEB_CT_INCOMING : 0u);
    // one `now` per call, from a monotonic clock: the max is the reference's overwrite, whatever
    // the order of the lanes. The load first: of a flow's packets in a batch, one refreshes and the
    // others find it done, instead of every packet's atomic on the one word
    const uint64_t expires = now + ct_timeout(p, ct_key_protocol(k));
    if (m.load(&slots[s].expires) < expires) m.fetch_max(&slots[s].expires, expires);
    return NEB_CT_HIT;
}

// ---- add (addConn) ------------------------------------------------------------------------------

struct CtAdd {
    uint32_t code;  // NEB_CT_NEW, _EXISTING, _DUP or _FULL; between the two launches also kCtRefused
    uint32_t slot;  // kCtNoSlot with _FULL
};
// The first launch's answer of a claimer whose place in the table was gone when it counted itself in:
// its slot becomes a tombstone in the second launch, and it and its copies answer FULL.
constexpr uint32_t kCtRefused = 5;

// The first launch of an add, for element `index` of the batch. key_of(j): the canonical key of the
// batch's element j, which nothing writes while the launch runs; so a copy compares itself with the
// claimer's input and nobody reads a slot's key words before they are settled. live: the count of
// live entries. During the launch it only rises until the table is full and never falls below
// capacity after that (a refused claimer takes itself out again), so an element that reads it full
// and then still finds the slot EMPTY answers FULL without a claim, and so do all copies of its key:
// one that claims later counts itself in later, and is refused. A full table therefore stays as it is; only claimers
// that were on their way while the last place went leave a tombstone. Nothing here waits for
// another element: a failed claim looks at the same slot again, which by then is CLAIMED for good.
template <class M, class KeyOf>
NEB_RT_HD CtAdd ct_add_claim(CtSlot* slots, uint64_t* live, const CtParams& p, uint32_t version, uint64_t now, uint32_t index,
                             const CtKey& k, uint32_t incoming, KeyOf key_of, M m) {
    const uint64_t h = ct_hash(p.seed, k);
    const uint32_t fp = ct_fp(h);
    const uint64_t expires = now + ct_timeout(p, ct_key_protocol(k));
    const uint64_t meta = ct_meta_in_add(index, version, incoming);
    uint32_t s = ct_home(h, p.mask);
    for (uint32_t n = 0; n <= p.mask; n++, s = (s + 1u) & p.mask) {
        uint64_t st = m.load(&slots[s].state);
        if (st == kCtEmpty) {
            // Full: the slot is looked at once more, behind the count. Still EMPTY: whoever claims it
            // from now on counts itself in later still and is refused, so FULL is every copy's answer.
            // Taken meanwhile, perhaps by a copy of this key that got the last place: compare below.
            const bool full = m.load(live) >= p.capacity;
            st = full ? m.load(&slots[s].state) : m.cas(&slots[s].state, kCtEmpty, ct_claimed(index, fp));
            if (st == kCtEmpty) {
                if (full) break;
                if (m.fetch_add(live, 1) >= p.capacity) {
                    m.fetch_sub(live, 1);
                    return CtAdd{kCtRefused, s};
                }
                for (int i = 0; i < 5; i++) m.store(&slots[s].key[i], k.w[i]);
                m.store(&slots[s].expires, expires);
                m.fetch_max(&slots[s].meta, meta);
                return CtAdd{NEB_CT_NEW, s};
            }
        }
        if ((st & kCtKindMask) == kCtClaimed && ct_state_fp(st) == fp) {
            if (ct_key_eq(key_of(ct_state_owner(st)), k)) {
                m.fetch_max(&slots[s].meta, meta);
                return CtAdd{NEB_CT_DUP, s};
            }
        } else if (st == ct_settled(fp) && ct_key_eq(ct_slot_key(&slots[s], m), k)) {
            // the copy that finds the settled word untouched overwrites the entry; the others follow it
            const bool first = (m.fetch_max(&slots[s].meta, meta) >> 32) == 0;
            if (first) m.store(&slots[s].expires, expires);
            return CtAdd{first ? (uint32_t)NEB_CT_EXISTING : (uint32_t)NEB_CT_DUP, s};
        }
    }
    return CtAdd{NEB_CT_FULL, kCtNoSlot};  // the table is full, or the chain has no EMPTY slot left
}

// The second launch, over the results of the first -> the element's final answer. The claimer
// publishes its slot, or buries it when it was refused; whoever answered NEW or EXISTING (one per
// key) takes the batch index out of meta; a copy follows its claimer. code_of(j): the code of
// element j as either launch wrote it: a claimer's is NEW from first to last, or kCtRefused and then
// FULL, so a copy that still finds the slot CLAIMED reads its claimer's fate whichever it sees.
template <class M, class CodeOf>
NEB_RT_HD CtAdd ct_add_settle(CtSlot* slots, uint64_t* counters, const CtAdd& r, CodeOf code_of, M m) {
    if (r.code == NEB_CT_FULL) return r;
    CtSlot* s = &slots[r.slot];
    if (r.code == kCtRefused) {
        m.store(&s->state, kCtTomb);
        m.fetch_add(&counters[1], 1);
        return CtAdd{NEB_CT_FULL, kCtNoSlot};
    }
    if (r.code == NEB_CT_DUP) {
        const uint64_t st = m.load(&s->state);
        const bool refused = (st & kCtKindMask) == kCtClaimed ? code_of(ct_state_owner(st)) != NEB_CT_NEW : st == kCtTomb;
        return refused ? CtAdd{NEB_CT_FULL, kCtNoSlot} : r;
    }
    m.store(&s->meta, m.load(&s->meta) & 0xFFFFFFFFull);
    if (r.code == NEB_CT_NEW) m.store_release(&s->state, ct_settled(ct_state_fp(m.load(&s->state))));
    return r;
}

// ---- evict ----------------------------------------------------------------------------------------

// -1: absent; > 0: the ns the entry still has (it stays); 0: removed. counters: {live, tombstones}.
template <class M>
NEB_RT_HD int64_t ct_evict_one(CtSlot* slots, uint64_t* counters, const CtParams& p, uint64_t now, bool force, const CtKey& k, M m) {
    const uint64_t h = ct_hash(p.seed, k);
    uint32_t s;
    if (!ct_find(slots, p, k, h, m, &s)) return -1;
    const uint64_t expires = m.load(&slots[s].expires);
    if (!force && expires > now) return (int64_t)(expires - now);
    // a copy of the key in the same batch may have been here first: it found the entry as well
    if (m.cas(&slots[s].state, ct_settled(ct_fp(h)), kCtTomb) == ct_settled(ct_fp(h))) {
        m.fetch_sub(&counters[0], 1);
        m.fetch_add(&counters[1], 1);
    }
    return 0;
}

// ---- compaction -----------------------------------------------------------------------------------

// One settled slot of the old image into the cleared new one. The old image's keys are distinct and
// nothing else runs, so a claim publishes at once and no key word is read.
template <class M>
NEB_RT_HD void ct_rehash_one(const CtSlot* old_slot, CtSlot* slots, const CtParams& p, M m) {
    const uint64_t st = m.load(&old_slot->state);
    if ((st & kCtKindMask) != kCtSettled) return;
    const CtKey k = ct_slot_key(old_slot, m);
    const uint64_t h = ct_hash(p.seed, k);
    uint32_t s = ct_home(h, p.mask);
    for (uint32_t n = 0; n <= p.mask; n++, s = (s + 1u) & p.mask) {
        if (m.load(&slots[s].state) != kCtEmpty) continue;
        if (m.cas(&slots[s].state, kCtEmpty, ct_settled(ct_fp(h))) != kCtEmpty) continue;
        for (int i = 0; i < 5; i++) m.store(&slots[s].key[i], k.w[i]);
        m.store(&slots[s].expires, m.load(&old_slot->expires));
        m.store(&slots[s].meta, m.load(&old_slot->meta));
        return;
    }
}

// ---- the host's memory policy -------------------------------------------------------------------

struct CtHostMem {
    uint64_t load(const uint64_t* p) const { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
    void store(uint64_t* p, uint64_t v) const { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
    void store_release(uint64_t* p, uint64_t v) const { __atomic_store_n(p, v, __ATOMIC_RELEASE); }
    uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) const {
        __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE);
        return expect;
    }
    uint64_t fetch_add(uint64_t* p, uint64_t v) const { return __atomic_fetch_add(p, v, __ATOMIC_ACQ_REL); }
    uint64_t fetch_sub(uint64_t* p, uint64_t v) const { return __atomic_fetch_sub(p, v, __ATOMIC_ACQ_REL); }
    uint64_t fetch_max(uint64_t* p, uint64_t v) const {
        uint64_t old = __atomic_load_n(p, __ATOMIC_RELAXED);
        while (old < v && !__atomic_compare_exchange_n(p, &old, v, true, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED)) {
        }
        return old;
    }
};

// A neb_fw_packet of any alignment as its six words.
inline CtKey ct_key_of(const neb_fw_packet* fw) {
    uint64_t q[6];
    __builtin_memcpy(q, fw, sizeof q);
    return ct_key_from_words(q);
}

}  // namespace neb
