"""Directed cases of the connection table (neb_conntrack_*), as scripts for conntrack_ref.play: the
chains that collide, wrap and pass tombstones are found with neb_conntrack_home on a host-only table
of the same seed and capacity, so they are the same chains on the device. Each case names what it is
there to reach; `reached(ct)` asserts on the table a runner has just played it on that it did."""
import numpy as np

from nebula_amd import _lib as L
from nebula_amd import firewall as F

import conntrack_ref as R

SEED = 0x5EED0C0FFEE
T0 = 1_000_000_000_000  # ns
OK = L.STATUS_OK
_probes = {}


def probe(capacity):
    if capacity not in _probes:
        _probes[capacity] = F.Conntrack(None, capacity, seed=SEED, max_batch=1024)
    return _probes[capacity]


def udp(rport, lport=4242, la="10.0.0.1", ra="10.0.0.2", proto=17):
    return F.fw_packets([(la, ra, lport, rport, proto)])


def homed(capacity, home, count, start=1):
    """`count` UDP keys (differing in the remote port) whose home slot is `home`."""
    p, out, port = probe(capacity), [], start
    while len(out) < count:
        k = udp(port)
        if p.home(k) == home:
            out.append(k)
        port += 1
        assert port < 65536
    return np.concatenate(out)


def cat(*a):
    return np.concatenate(a)


def look(fw, now=T0, status=None, hold=None, work_cap=None):
    return ("lookup", fw, [OK] * len(fw) if status is None else status, now, hold, work_cap)


class Case:
    def __init__(self, name, capacity, steps, reached, device=True, max_batch=1024):
        self.name, self.capacity, self.steps, self.reached, self.device, self.max_batch = \
            name, capacity, steps, reached, device, max_batch

    def __repr__(self):
        return self.name


def slots_of(ct, fw):
    e = ct.entries()
    return [e[k][3] for k in R.keys_of(fw)]


def states(ct):
    return [int(s) for s in ct.dump()["state"]]


def case_collide():
    k = homed(4, 2, 3)

    def reached(ct):
        assert [ct.home(k[i]) for i in range(3)] == [2, 2, 2]
        assert sorted(slots_of(ct, k)) == [2, 3, 4]
    return Case("three keys, one home slot", 4, [("add", k, [0, 1, 0], T0), look(k), look(k[::-1].copy(), T0 + 5)], reached)


def case_wrap():
    k = homed(4, 7, 3)

    def reached(ct):
        assert sorted(slots_of(ct, k)) == [0, 1, 7]
    return Case("a chain that wraps past the last slot", 4, [("add", k, [0, 0, 1], T0), look(k)], reached)


def case_tombstones():
    k = homed(4, 5, 3)  # a, b live in 5 and 6; c is never added

    def reached(ct):
        st = states(ct)
        assert st[5] == L.CT_STATE_TOMB and slots_of(ct, k[1:2]) == [6] and st[7] == L.CT_STATE_EMPTY
        assert ct.count()[:2] == (1, 1)
    steps = [("add", k[:1], [0], T0), ("add", k[1:2], [0], T0),  # one after the other: a sits in the home slot
             ("evict", k[:1], T0, True),
             look(k[1:2]),  # found behind a tombstone
             look(k[2:3]),  # absent: the chain passes the tombstone and b, and ends at EMPTY
             look(k[:1])]   # the evicted key misses
    return Case("a key behind a tombstone, an absent key past one", 4, steps, reached)


def one_field_variants():
    base4 = F.fw_packets([("10.1.2.3", "10.4.5.6", 1000, 2000, 6)])
    base6 = F.fw_packets([("fd00::1:2:3", "fd00::4:5:6", 1000, 2000, 6)])
    out = []

    def vary(base, fn):
        v = base.copy()
        fn(v[0])
        out.append(v)

    def flip(field, byte):
        def f(r):
            r[field][byte] ^= 0x10
        return f

    for base in (base4, base6):
        vary(base, lambda r: r.__setitem__("local_port", 1001))
        vary(base, lambda r: r.__setitem__("remote_port", 2001))
        vary(base, lambda r: r.__setitem__("protocol", 17))
        vary(base, lambda r: r.__setitem__("flags", L.FW_FRAGMENT))
        for field in ("local_addr", "remote_addr"):
            vary(base, flip(field, 0))
            vary(base, flip(field, 3))
    for field in ("local_addr", "remote_addr"):
        vary(base6, flip(field, 4))
        vary(base6, flip(field, 15))
    # family alone: the same 16 address bytes (the leading four, the rest zero) as family 4 and 6
    fam6 = base4.copy()
    fam6[0]["family"] = 6
    out.append(fam6)
    return base4, base6, np.concatenate(out)


def case_one_field():
    b4, b6, var = one_field_variants()
    allk = cat(b4, b6, var)

    def reached(ct):
        assert len(set(R.keys_of(allk))) == len(allk) == ct.count()[0]
    steps = [("add", cat(b4, b6), [0, 1], T0), look(allk),  # the two bases hit, every variant misses
             ("add", var, [0] * len(var), T0), look(allk)]
    return Case("keys differing in exactly one field", 32, steps, reached)


def case_not_key_fields():
    """ip_hdr_len, gateway, the other flag bits and the reserved fields are not part of the key; nor
    are bytes 4..15 of a family-4 address."""
    clean = F.fw_packets([("10.1.2.3", "10.4.5.6", 1000, 2000, 6)])
    dirty = clean.copy()
    dirty[0]["local_addr"][4:] = 0xA5
    dirty[0]["remote_addr"][4:] = np.arange(12) + 1
    dirty[0]["flags"] = L.FW_FRAG_ANY | L.FW_ROUTED | L.FW_ECMP_FALLBACK
    dirty[0]["reserved"], dirty[0]["reserved2"], dirty[0]["ip_hdr_len"], dirty[0]["gateway"] = 7, 9, 20, 3

    def reached(ct):
        assert ct.count()[0] == 1 and R.keys_of(clean) == R.keys_of(dirty) and clean.tobytes() != dirty.tobytes()
    return Case("v4 keys whose input bytes 4..15 are garbage", 4,
                [("add", clean, [1], T0), look(dirty), ("add", dirty, [0], T0 + 1), look(cat(clean, dirty), T0 + 2)], reached)


def case_4in6():
    v4 = F.fw_packets([("1.2.3.4", "1.2.3.5", 10, 90, 17)])
    m6 = F.fw_packets([("::ffff:1.2.3.4", "::ffff:1.2.3.5", 10, 90, 17)])

    def reached(ct):
        assert ct.count()[0] == 2
    return Case("4-in-6 against v4", 4, [("add", v4, [0], T0), look(cat(v4, m6)), ("add", m6, [0], T0), look(cat(v4, m6))],
                reached)


def case_icmp():
    a = F.fw_packets([("10.0.0.1", "10.0.0.2", 0, 0x1234, 1), ("10.0.0.1", "10.0.0.2", 0, 0x1235, 1),
                      ("fd00::1", "fd00::2", 0, 0x1234, 58)])

    def reached(ct):
        assert all(v[0] == T0 + R.DEFAULT_NS for v in ct.entries().values())
    return Case("ICMP with identifier", 4, [("add", a[:1], [1], T0), look(a), ("add", a[2:], [1], T0), look(a)], reached)


def case_timeouts():
    a = F.fw_packets([("10.0.0.1", "10.0.0.2", 1, 2, 6), ("10.0.0.1", "10.0.0.2", 1, 2, 17), ("10.0.0.1", "10.0.0.2", 1, 2, 47)])

    def reached(ct):
        e = ct.entries()
        assert [e[k][0] - (T0 + 9) for k in R.keys_of(a)] == [R.TCP_NS, R.UDP_NS, R.DEFAULT_NS]
    return Case("TCP, UDP and other: the three timeouts", 4, [("add", a, [0, 0, 0], T0), look(a, T0 + 9)], reached)


def case_expires():
    a = udp(53)
    late = T0 + 10 * R.UDP_NS

    def reached(ct):
        assert list(ct.entries().values())[0][0] == late + R.UDP_NS
    steps = [("add", a, [0], T0),
             look(a, T0 - 5),  # HIT with Expires already larger: the max keeps it
             ("evict", a, T0 + 1, False),  # > 0: proves it kept T0 + UDP_NS
             look(a, late)]  # long past Expires and never evicted: still hits, and is refreshed
    return Case("HIT keeps a larger Expires; a past-Expires entry still hits", 4, steps, reached)


def case_stale():
    a = cat(udp(1), udp(2))

    def reached(ct):
        assert sorted(v[1:3] for v in ct.entries().values()) == [(0, 0), (1, 0)]
    steps = [("version", 65535), ("add", a, [0, 1], T0), look(a), ("version", 0),  # 65535 -> 0: the version wraps
             look(a, T0 + 7, hold="rx"),  # STALE, STALE | INCOMING: the entries untouched
             ("add", a, [0, 1], T0 + 8), look(a, T0 + 9)]
    return Case("STALE with incoming 0 and 1, and the version wrap", 4, steps, reached)


def case_add_codes():
    a, b = udp(1), udp(2)
    wave = np.repeat(udp(3), 64)
    inc64 = [i & 1 for i in range(64)]  # the last copy: incoming
    many = np.repeat(udp(4), 600)  # copies across three workgroups
    inc600 = [1] * 599 + [0]

    def reached(ct):
        e = ct.entries()
        assert e[R.keys_of(wave)[0]][1] == 0 and e[R.keys_of(many)[0]][1] == 1 and len(e) == 4  # the last add's copies
    steps = [("add", cat(a, b, a), [0, 1, 1], T0), ("add", a, [0], T0 + 1), ("add", wave, inc64, T0 + 2),
             ("add", many, inc600, T0 + 3), ("add", cat(wave[:3], many[:2], b), [0, 0, 0, 1, 1, 0], T0 + 4),
             look(cat(a, b, wave[:1], many[:1]), T0 + 5)]
    return Case("add: NEW, EXISTING, DUP; 64 copies in one wave; copies across workgroups", 8, steps, reached)


def case_full_capacity():
    k = cat(*[udp(p) for p in range(1, 7)])

    def reached(ct):
        assert ct.count()[0] == 4
    steps = [("add", k, [0] * 6, T0), look(k), ("add", k[4:], [0, 0], T0 + 1), ("evict", k[:1], T0, True),
             ("add", k[4:], [1, 1], T0 + 2), look(k)]
    return Case("FULL by capacity", 4, steps, reached, device=False)  # which keys the device refuses is unspecified: tests/test_gpu_conntrack.py plays it by its invariants


def case_full_tombstones():
    k = cat(*[udp(p) for p in range(1, 10)])

    def reached(ct):
        assert ct.count() == (1, 0, 8)
    steps = [("add", k[:4], [0] * 4, T0), ("evict", k[:4], T0, True), ("add", k[4:8], [0] * 4, T0), ("evict", k[4:8], T0, True),
             ("add", k[8:], [1], T0, True),  # eight tombstones, nothing live: no EMPTY slot, FULL
             look(k[8:]), ("compact",), ("add", k[8:], [1], T0), look(k)]
    return Case("FULL by tombstones", 4, steps, reached)


def case_evict():
    a, b, c, d = udp(1), udp(2), udp(3), udp(4)

    def reached(ct):
        assert ct.count()[:2] == (1, 4)
    steps = [("add", cat(a, b, c), [0, 0, 0], T0),
             ("evict", cat(d, a), T0 + 1, False),  # -1 (absent); > 0 (stays)
             ("evict", a, T0 + R.UDP_NS, False),  # Expires == now: 0
             ("evict", b, T0 + 1, True),  # forced
             look(cat(a, b, c)),
             ("add", d, [0], T0), ("evict", cat(d, d, c), T0 + R.UDP_NS + 1, False),  # a duplicated key
             ("add", d, [1], T0 + 2)]
    return Case("evict: -1, > 0, 0, forced, a duplicated key", 4, steps, reached)


def case_compact():
    k = homed(4, 1, 4)

    def reached(ct):
        assert sorted(slots_of(ct, k[2:])) == [1, 2] and slots_of(ct, k[:1]) == [3] and ct.count()[:2] == (3, 0)
    steps = [("add", k, [0, 1, 0, 1], T0), ("evict", k[:2], T0, True), look(k), ("compact",), look(k, T0 + 1),
             ("add", k[:1], [1], T0 + 2), look(k, T0 + 3)]
    return Case("compaction keeps the live entries and moves them", 4, steps, reached)


def case_status():
    k = cat(udp(1), udp(2), udp(1), udp(2), udp(3))
    st = [OK, L.STATUS_AUTH_FAILED, L.STATUS_INVALID, OK, L.STATUS_RX_BAD_LOCAL]
    steps = [("add", k[:1], [0], T0), look(k, T0, st, "rx"), look(k, T0, st, "tx"), look(k, T0, st, None)]
    return Case("inputs with status != OK are not looked up and not held", 4, steps, lambda ct: None)


def case_work_cap():
    k = cat(*[udp(p) for p in range(1, 8)])
    steps = [("add", k[2:4], [0, 0], T0), look(k, T0, None, "tx", 2), look(k, T0, None, "rx", 0), look(k, T0, None, None, 5),
             look(k[2:4], T0, None, "rx", 0)]
    return Case("work_cap smaller than the work count", 4, steps, lambda ct: None)


def case_capacity_one():
    a, b = udp(1), udp(2)

    def reached(ct):
        assert ct.count() == (1, 0, 2)
    steps = [("add", a, [0], T0), look(cat(a, b)), ("evict", a, T0, True), ("add", b, [1], T0), look(cat(a, b)), ("compact",),
             look(cat(a, b))]
    return Case("capacity 1: two slots", 1, steps, reached)


def all_cases():
    return [case_collide(), case_wrap(), case_tombstones(), case_one_field(), case_not_key_fields(), case_4in6(), case_icmp(),
            case_timeouts(), case_expires(), case_stale(), case_add_codes(), case_full_capacity(), case_full_tombstones(),
            case_evict(), case_compact(), case_status(), case_work_cap(), case_capacity_one()]


# ---- random scripts ----------------------------------------------------------------------------------

def universe(n):
    """n distinct keys of mixed families and protocols."""
    rows = []
    for i in range(n):
        proto = (6, 17, 1)[i % 3]
        if i % 4 == 3:
            rows.append((f"fd00::{i + 1:x}", "fd00::ffff", 100 + i, 200, proto))
        else:
            rows.append((f"10.0.{i >> 8}.{i & 255}", "10.9.9.9", 100 + (i % 7), 200 + i % 65000, proto))
    return F.fw_packets(rows)


def random_script(rng, model, runner, keys, nsteps, sizes):
    """Plays random steps of mixed operations with batch sizes from `sizes`; compacts before an add
    that might otherwise find no EMPTY slot (which the model does not know about)."""
    ct = runner.ct
    now = T0
    for step in range(nsteps):
        n = int(rng.choice(sizes))
        pick = keys[rng.integers(0, len(keys), n)]
        now += int(rng.integers(0, R.UDP_NS // 2))
        op = rng.integers(0, 10)
        if op < 4:
            status = [OK if rng.random() < 0.9 else L.STATUS_REPLAY for _ in range(n)]
            hold = (None, "rx", "tx")[int(rng.integers(0, 3))]
            cap = (None, 0, n // 2)[int(rng.integers(0, 3))]
            R.play([("lookup", pick, status, now, hold, cap)], model, runner)
        elif op < 7:
            _, tombs, slots = ct.count()
            if tombs >= slots - ct.capacity:
                R.play([("compact",)], model, runner)
            R.play([("add", pick, [int(b) for b in rng.integers(0, 2, n)], now)], model, runner)
        elif op < 9:
            R.play([("evict", pick, now, bool(rng.random() < 0.3))], model, runner)
        else:
            R.play([("version", int(rng.integers(0, 3)))], model, runner)
