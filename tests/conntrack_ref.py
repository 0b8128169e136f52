"""A model of firewall.Conntrack.Conns as the connection table keeps it (neb_conntrack_*,
include/nebula_aead.h), written from the reference's text (firewall.go:30-38, 505-630): a dict from
the canonical key to [Expires, incoming, rulesVersion] with inConns, addConn and evict over whole
batches, in array order. And a toy firewall over it, with the two ways to drive it: packet by packet
as firewall.Drop does, and batch-wise as a caller of the table does (lookup -> rules over the work
list -> add), which must agree on every packet and leave the same map.

Also the runner that plays one script of steps on the model and on a table (host-only or device) and
compares everything either returns, used by the host and the GPU tests."""
import numpy as np

from nebula_amd import _lib as L
from nebula_amd import firewall as F

TCP_NS, UDP_NS, DEFAULT_NS = 12 * 60 * 10**9, 3 * 60 * 10**9, 10 * 60 * 10**9


def keys_of(fw):
    """FW_PACKET_DTYPE records -> the canonical keys, hashable."""
    return [tuple(int(w) for w in row) for row in F.key_words(fw)]


def key_protocol(key):
    return (key[4] >> 32) & 0xFF


class Model:
    def __init__(self, capacity, tcp_ns=TCP_NS, udp_ns=UDP_NS, default_ns=DEFAULT_NS):
        self.capacity = capacity
        self.timeouts = (tcp_ns, udp_ns, default_ns)
        self.version = 0
        self.conns = {}  # key -> [expires, incoming, version]

    def timeout(self, key):
        p = key_protocol(key)
        return self.timeouts[0] if p == 6 else self.timeouts[1] if p == 17 else self.timeouts[2]

    def set_rules_version(self, v):
        self.version = v & 0xFFFF

    def lookup(self, fw, status, now):
        """-> (verdict per packet, [(packet, verdict)] of the work list, counts[4])"""
        verdict, work, counts = [], [], [0, 0, 0, 0]
        for i, key in enumerate(keys_of(fw)):
            if status[i] != L.STATUS_OK:
                verdict.append(L.CT_NONE)
                continue
            c = self.conns.get(key)
            if c is None:
                v = L.CT_MISS
            elif c[2] != self.version:
                v = L.CT_STALE | (L.CT_INCOMING if c[1] else 0)
            else:
                v = L.CT_HIT
                c[0] = max(c[0], now + self.timeout(key))
            counts[(v & 0x7F) - 1] += 1
            if v != L.CT_HIT:
                work.append((i, v))
            verdict.append(v)
        counts[3] = len(work)
        return verdict, work, counts

    def add(self, fw, incoming, now, full=False):
        """-> codes. full: every new key is refused (the image has no EMPTY slot left, which the
        model does not know about)."""
        codes, seen = [], set()
        for key, inc in zip(keys_of(fw), incoming):
            if key in seen:
                codes.append(L.CT_DUP)
                self.conns[key][1] = int(bool(inc))
                continue
            if key in self.conns:
                codes.append(L.CT_EXISTING)
            elif full or len(self.conns) >= self.capacity:
                codes.append(L.CT_FULL)
                continue
            else:
                codes.append(L.CT_NEW)
            seen.add(key)
            self.conns[key] = [now + self.timeout(key), int(bool(inc)), self.version]
        return codes

    def evict(self, fw, now, force=False):
        out = []
        for key in keys_of(fw):
            c = self.conns.get(key)
            if c is None:
                out.append(-1)
            elif c[0] > now and not force:
                out.append(c[0] - now)
            else:
                del self.conns[key]
                out.append(0)
        return out

    def snapshot(self):
        return {k: tuple(v) for k, v in self.conns.items()}


class HostTableAsModel:
    """A host-only table behind the model's interface, for the toy firewall."""

    def __init__(self, ct):
        self.ct, self.version = ct, 0

    def set_rules_version(self, v):
        self.version = v & 0xFFFF
        self.ct.set_rules_version(v)

    def lookup(self, fw, status, now):
        verdict, work, counts = self.ct.lookup_host(fw, np.array(status, np.int32), now)
        return [int(v) for v in verdict], [(int(w["packet"]), int(w["verdict"])) for w in work], [int(c) for c in counts]

    def add(self, fw, incoming, now):
        return [int(c) for c in self.ct.add_host(fw, [int(bool(b)) for b in incoming], now)["code"]]

    def evict(self, fw, now, force=False):
        return [int(r) for r in self.ct.evict_host(fw, now, force)]

    def snapshot(self):
        return table_snapshot(self.ct)


# ---- the toy firewall ------------------------------------------------------------------------------

class ToyFirewall:
    """rules: a set of (incoming, protocol or 0 for any, port or 0 for any); the port of a packet is
    its local port when incoming, else its remote port. wheel: the keys the caller would have to put
    on its timer wheel, in order."""

    def __init__(self, model, rules):
        self.ct, self.rules, self.wheel = model, set(rules), []

    def match(self, rec, incoming):
        port = int(rec["local_port"] if incoming else rec["remote_port"])
        proto = int(rec["protocol"])
        return any(d == bool(incoming) and p in (0, proto) and q in (0, port) for d, p, q in self.rules)

    def reload(self, rules):
        self.rules = set(rules)
        self.ct.set_rules_version(self.ct.version + 1)

    def drop_packet(self, rec, incoming, now):
        """firewall.Drop from inConns on (firewall.go:459-478) for one packet -> passes."""
        one = np.array([rec], L.FW_PACKET_DTYPE)
        v = self.ct.lookup(one, [L.STATUS_OK], now)[0][0]
        if v == L.CT_HIT:
            return True
        if (v & 0x7F) == L.CT_STALE:
            was_incoming = bool(v & L.CT_INCOMING)
            if self.match(rec, was_incoming):  # firewall.go:559-569: the entry is brought up to date
                self.ct.add(one, [was_incoming], now)
                return True
            self.ct.evict(one, now, force=True)  # firewall.go:545
        if not self.match(rec, incoming):
            return False
        if self.ct.add(one, [incoming], now)[0] == L.CT_NEW:
            self.wheel.append(keys_of(one)[0])
        return True

    def drop_batch(self, fw, incoming, now):
        """The same for a batch of one direction: one lookup, the rules over the work list, one
        evict and one add -> passes per packet."""
        n = len(fw)
        verdict, work, _ = self.ct.lookup(fw, [L.STATUS_OK] * n, now)
        passes = [v == L.CT_HIT for v in verdict]
        keys = keys_of(fw)
        decided = {}  # key -> (passes, add as incoming or None, evict)
        for i, v in work:
            if keys[i] in decided:
                continue
            evict, add = False, None
            if (v & 0x7F) == L.CT_STALE:
                was_incoming = bool(v & L.CT_INCOMING)
                if self.match(fw[i], was_incoming):
                    add = was_incoming
                else:
                    evict = True
            if add is None and self.match(fw[i], incoming):
                add = bool(incoming)
            decided[keys[i]] = (add is not None, add, evict, i)
        ev = [d[3] for d in decided.values() if d[2]]
        if ev:
            self.ct.evict(fw[ev], now, force=True)
        ad = [d[3] for d in decided.values() if d[1] is not None]
        if ad:
            codes = self.ct.add(fw[ad], [decided[keys[i]][1] for i in ad], now)
            self.wheel += [keys[i] for i, c in zip(ad, codes) if c == L.CT_NEW]
        for i, _ in work:
            passes[i] = decided[keys[i]][0]
        return passes


# ---- one script on the model and on a table --------------------------------------------------------

def table_snapshot(ct):
    return {k: v[:3] for k, v in ct.entries().items()}


def groups(keys):
    g = {}
    for i, k in enumerate(keys):
        g.setdefault(k, []).append(i)
    return g


def check_add(keys, model_codes, res, exact):
    """exact: the table adds in array order too (the host form) and answers as the model does, copy
    by copy. Otherwise, per key: the same codes as a multiset, and one slot."""
    codes = [int(c) for c in res["code"]]
    if exact:
        assert codes == model_codes, (codes, model_codes)
    for k, idx in groups(keys).items():
        assert sorted(codes[i] for i in idx) == sorted(model_codes[i] for i in idx), (k, idx)
        assert len({int(res["slot"][i]) for i in idx}) == 1
        assert all((int(res["slot"][i]) == L.CT_NO_SLOT) == (codes[i] == L.CT_FULL) for i in idx)


def check_evict(keys, model_rem, rem, exact):
    rem = [int(r) for r in rem]
    if exact:
        assert rem == model_rem, (rem, model_rem)
    for k, idx in groups(keys).items():
        want = [model_rem[i] for i in idx]
        got = [rem[i] for i in idx]
        if 0 in want:  # removed: every copy found it there (0) or gone (-1), and one removed it
            assert set(got) <= {0, -1} and 0 in got, (k, got)
        else:
            assert got == want, (k, got, want)


class HostRunner:
    """Plays steps on a host-only table. A device runner (tests/test_gpu_conntrack.py) has the same
    methods over device memory."""
    exact = True

    def __init__(self, ct):
        self.ct = ct

    def lookup(self, fw, status, now, hold, work_cap):
        status = np.array(status, np.int32)
        plain = tx = None
        if hold == "rx":
            plain = np.zeros(len(fw), L.PLAIN_PACKET_DTYPE)
            plain["flags"] = L.PLAIN_PARSED
        if hold == "tx":
            from nebula_amd.inside import TX_PACKET_DTYPE

            tx = np.zeros(len(fw), TX_PACKET_DTYPE)
            tx["tunnel"] = np.arange(len(fw))
        verdict, work, counts = self.ct.lookup_host(fw, status, now, plain=plain, tx=tx, work_cap=work_cap)
        return verdict, work, counts, status, plain, tx

    def add(self, fw, incoming, now):
        return self.ct.add_host(fw, incoming, now)

    def evict(self, fw, now, force):
        return self.ct.evict_host(fw, now, force)


def play(steps, model, runner, after_step=None):
    """steps: ("version", v) | ("lookup", fw, status, now, hold, work_cap) | ("add", fw, incoming, now[,
    full]) | ("evict", fw, now, force) | ("compact",). Asserts that the table answers as the model
    does and holds the model's map after every step."""
    ct = runner.ct
    for step in steps:
        op = step[0]
        if op == "version":
            model.set_rules_version(step[1])
            ct.set_rules_version(step[1])
        elif op == "lookup":
            _, fw, status, now, hold, work_cap = step
            n = len(fw)
            mv, mwork, mcounts = model.lookup(fw, status, now)
            verdict, work, counts, st, plain, tx = runner.lookup(fw, status, now, hold, work_cap)
            assert [int(v) for v in verdict] == mv
            assert [int(c) for c in counts] == mcounts
            cap = n if work_cap is None else work_cap
            assert len(work) == min(len(mwork), cap)
            assert [(int(w["packet"]), int(w["verdict"])) for w in work] == mwork[:cap]  # ascending packet order
            for w in work:
                assert w["fw"].tobytes() == fw[int(w["packet"])].tobytes() and not w["reserved"].any()
            held = [v not in (L.CT_NONE, L.CT_HIT) for v in mv]
            want_st = [L.STATUS_FW_HELD if (h and hold) else s for h, s in zip(held, status)]
            assert [int(s) for s in st] == want_st
            if plain is not None:
                assert [int(f) for f in plain["flags"]] == [L.PLAIN_PARSED | (L.PLAIN_SKIP if h else 0) for h in held]
            if tx is not None:
                assert [int(t) for t in tx["tunnel"]] == [L.TX_NO_TUNNEL if h else i for i, h in enumerate(held)]
        elif op == "add":
            fw, incoming, now = step[1:4]
            full = len(step) > 4 and step[4]
            check_add(keys_of(fw), model.add(fw, incoming, now, full=full), runner.add(fw, incoming, now), runner.exact)
        elif op == "evict":
            _, fw, now, force = step
            check_evict(keys_of(fw), model.evict(fw, now, force), runner.evict(fw, now, force), runner.exact)
        elif op == "compact":
            before = ct.dump()
            ct.compact()
            assert ct.count()[1] == 0
            if after_step:
                after_step(step, before)
        else:
            raise ValueError(op)
        assert table_snapshot(ct) == model.snapshot(), op
        assert ct.count()[0] == len(model.conns)
