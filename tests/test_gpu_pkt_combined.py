"""GPU: the combined per-packet launch (aes_gcm.hip gcm_one_batch_kernel: one request per wave, four
waves per workgroup, each wave its own key tables and its own copy of its slot in LDS), bit for bit
against the CPU oracle, through neb_engine_pkt_launch: request r of a call rides in slot r of one
launch, so which shape, key and forgery sits in which wave of which workgroup is the test's choice
and not a matter of thread timing. The cases and what they cover are tests/pkt_combined_cases.py
(checked on the CPU by tests/test_pkt_combined_cases.py).

Every directed launch follows a launch whose 32 requests fill their slots to the limit with
non-zero bytes (the engine reuses its batch buffers, last in first out), so the padding behind an
odd AAD and the bytes behind a short payload are stale, never zero. Every output lies at a byte
skew of its own inside a guarded host buffer: no byte outside [out, out + out_len) may change.
The last test checks that neb_engine_pkt_combined rose by exactly the launches and requests this
file made: every one of them ran the combined kernel.
"""
from dataclasses import dataclass

import numpy as np
import pytest

import auth_cases as A
import pkt_combined_cases as P
from nebula_amd import _lib as L
from nebula_amd import noiseutil as N

pytestmark = pytest.mark.gpu

GUARD = 0xC3
OUT_STRIDE = 2304  # per request: 64 guard bytes, the output at a skew of 0..15, guard bytes
MADE = {"launches": 0, "calls": 0}  # what this file sent through neb_engine_pkt_launch


@pytest.fixture(scope="module", autouse=True)
def _combined_before(engine):
    s = engine.stats()
    MADE.update(launches=0, calls=0, base=(s["pkt_combined_launches"], s["pkt_combined_calls"]))


@dataclass
class Tunnels:
    engine: object
    oracle: object
    keys: np.ndarray  # 32 bytes per installed AES-256-GCM key, by key index
    kid: list         # key index -> the engine's key slot
    chacha_kid: int   # a slot that holds a ChaCha20-Poly1305 key


@pytest.fixture
def tun(engine, oracle_mod):
    rng = np.random.default_rng(3232)
    keys = rng.integers(0, 256, 32 * P.COMB_MAX, dtype=np.uint8)
    cs = N.CipherAESGCM.CipherBatch(engine, [keys[32 * i:32 * i + 32].tobytes() for i in range(P.COMB_MAX)])
    cha = N.CipherChaChaPoly.Cipher(engine, bytes(range(32)))
    yield Tunnels(engine, oracle_mod, keys, [c.key_id for c in cs], cha.key_id)
    for c in cs + [cha]:
        c.destroy()


@dataclass
class Item:
    key: int            # key index (Tunnels.keys)
    counter: int
    aad: np.ndarray
    inp: np.ndarray     # plaintext (seal) or ciphertext + tag (open)
    raw_key: int = -1   # >= 0: this raw key slot instead (not an installed AES-256-GCM key)


def oracle_results(t, open_, items):
    """(status, outputs) of every item by the oracle (oracle.batch over the items laid out as an
    arena): the output bytes for NEB_STATUS_OK, zeros for a failed open, None otherwise (nothing
    is written). An item on a raw key slot is NEB_STATUS_BAD_KEY."""
    n, stride = len(items), 4352
    arena = np.zeros(n * stride, np.uint8)
    desc = np.zeros(n, L.DESC_DTYPE)
    for r, it in enumerate(items):
        base, p = r * stride, P.pay(len(it.aad))
        arena[base:base + len(it.aad)] = it.aad
        arena[base + p:base + p + len(it.inp)] = it.inp
        ln = len(it.inp) - (16 if open_ else 0)
        desc[r] = (base + p, base + p, base, it.counter, ln, len(it.aad), it.key, 0)
    live = np.array([r for r, it in enumerate(items) if it.raw_key < 0], np.int64)
    st = np.full(n, L.STATUS_BAD_KEY, np.int32)
    if len(live):
        st[live] = t.oracle.batch(L.ALG_AESGCM, 1 if open_ else 0, t.keys, desc[live], arena)
    outs = []
    for r in range(n):
        dst, out_len = int(desc["dst_off"][r]), int(desc["len"][r]) + (0 if open_ else 16)
        if st[r] == L.STATUS_OK:
            outs.append(arena[dst:dst + out_len].copy())
        elif open_ and st[r] == L.STATUS_AUTH_FAILED:
            outs.append(np.zeros(out_len, np.uint8))
        else:
            outs.append(None)
    return st, outs


def device_launch(t, open_, items, expect_rc=L.OK):
    """One neb_engine_pkt_launch of `items`: (rc, statuses, guarded output buffer, output views).
    Statuses start at -77 and the buffer at GUARD, output r at skew r mod 16."""
    n = len(items)
    buf = np.full((max(n, 1), OUT_STRIDE), GUARD, np.uint8)
    st = np.full(max(n, 1), -77, np.int32)
    views, reqs = [], []
    for r, it in enumerate(items):
        out_len = len(it.inp) + (-16 if open_ else 16)
        lo = 64 + r % 16
        views.append(buf[r, lo:lo + max(out_len, 0)])
        reqs.append((it.raw_key if it.raw_key >= 0 else t.kid[it.key], it.counter, it.aad, it.inp, views[-1]))
    rc = t.engine.pkt_launch(open_, reqs, st)
    assert rc == expect_rc, (rc, L.lib().neb_last_error())
    if rc == L.OK and n:
        MADE["launches"] += 1
        MADE["calls"] += n
    return rc, st[:n], buf, views


def stale_launch(t):
    """32 seals that fill their slots to the limit (2048 non-zero bytes and the tag behind them)."""
    rng = np.random.default_rng(MADE["launches"])
    items = [Item(r, 7000 + r, np.zeros(0, np.uint8), rng.integers(1, 256, 2048, dtype=np.uint8)) for r in range(P.COMB_MAX)]
    _, st, _, _ = device_launch(t, False, items)
    assert (st == L.STATUS_OK).all()


def check_launch(t, open_, items, name="", stale=True):
    """A stale launch, then `items` as one launch: statuses and outputs equal the oracle's, and
    nothing but each [out, out + out_len) changed. Returns (statuses, outputs) of the device."""
    st_exp, out_exp = oracle_results(t, open_, items)
    if stale:
        stale_launch(t)
    _, st, buf, views = device_launch(t, open_, items)
    exp = np.full_like(buf, GUARD)
    for r, o in enumerate(out_exp):
        if o is not None:
            exp[r, 64 + r % 16:64 + r % 16 + len(o)] = o
    wrong = np.flatnonzero(st != st_exp)
    assert len(wrong) == 0, (name, "status", [(int(r), int(st[r]), int(st_exp[r])) for r in wrong])
    bad = np.flatnonzero((buf != exp).any(axis=1))
    assert len(bad) == 0, (name, "output", [(int(r), len(items[r].aad), len(items[r].inp),
                                             (np.flatnonzero(buf[r] != exp[r])[[0, -1]] - 64 - r % 16).tolist())
                                            for r in bad])
    return st, [v.copy() for v in views]


def make_items(t, la, seed):
    """The launch's requests with random contents and counters: plaintext items, and for an open
    launch the oracle's sealed packets with every forgery applied. (plain, items to launch)"""
    rng = np.random.default_rng(seed)
    plain = []
    for q in la.reqs:
        ctr = int(rng.integers(0, 2**62))
        if q.special == "exhausted":
            ctr = L.REJECT_AFTER_MESSAGES
        plain.append(Item(q.key, ctr, rng.integers(0, 256, q.aad_len, dtype=np.uint8),
                          rng.integers(0, 256, q.len, dtype=np.uint8)))
    if not la.open:
        items = [Item(p.key, p.counter, p.aad, p.inp) for p in plain]
    else:
        # (the oracle seals past the counter limit only through seal(): batch() refuses it, as the device does)
        sealed = [np.frombuffer(t.oracle.seal(L.ALG_AESGCM, t.keys[32 * p.key:32 * p.key + 32].tobytes(),
                                              t.oracle.nonce(L.ALG_AESGCM, p.counter), p.aad.tobytes(),
                                              p.inp.tobytes()), np.uint8).copy() for p in plain]
        items = []
        for q, p, s in zip(la.reqs, plain, sealed):
            aad, ctr = p.aad.copy(), p.counter
            if q.forged.startswith("tag_bit_"):
                b = int(q.forged[8:])
                s[len(s) - 16 + b // 8] ^= 1 << (b % 8)
            elif q.forged == "aad_last_byte":
                aad[-1] ^= 0x5A
            elif q.forged == "ct_last_byte":
                s[len(s) - 17] ^= 0x80
            elif q.forged:
                raise AssertionError(q.forged)
            items.append(Item(p.key, ctr, aad, s))
    for q, it in zip(la.reqs, items):
        if q.special.startswith("key_"):
            it.raw_key = {"key_max_keys": t.engine.max_keys, "key_all_ones": 0xFFFFFFFF,
                          "key_chacha_slot": t.chacha_kid}[q.special]
    return plain, items


def run_case(t, la, seed):
    plain, items = make_items(t, la, seed)
    st, outs = check_launch(t, la.open, items, la.name)
    for r, q in enumerate(la.reqs):
        if la.open and q.forged:
            assert st[r] == L.STATUS_AUTH_FAILED and not outs[r].any(), (la.name, r, q)
        elif q.special.startswith("key_"):
            assert st[r] == L.STATUS_BAD_KEY, (la.name, r, q)
        elif q.special == "exhausted" and not la.open:
            assert st[r] == L.STATUS_EXHAUSTED, (la.name, r, q)
        else:
            assert st[r] == L.STATUS_OK, (la.name, r, q)
            if la.open:  # opening the oracle's packet gives the plaintext back
                assert np.array_equal(outs[r], plain[r].inp), (la.name, r, q)
    return st, outs


# ---- the cases -----------------------------------------------------------------------------------

def test_block_count_sweep(tun):
    """The 402 shapes of the one-packet kernels, 32 to a launch, a key per slot: sealed like the
    oracle, and the oracle's packets opened back to the plaintext."""
    for open_ in (False, True):
        for i, la in enumerate(P.sweep_launches(open_)):
            run_case(tun, la, 100 + i)


def test_slot_coverage(tun):
    """Every slot 0..31 holds, over these launches, each kind of request the slot conditions name
    (no AAD, odd AAD, empty and partial payloads, both slot limits, forged, clean beside forged)."""
    ls = P.slot_cover_launches()
    assert P.slot_conditions(ls) == []
    for i, la in enumerate(ls):
        run_case(tun, la, 200 + i)


def test_launch_sizes(tun):
    """n = 1, 2, 3, 4, 5, 31, 32: idle waves in the last workgroup, one workgroup, eight."""
    for i, la in enumerate(P.size_launches()):
        run_case(tun, la, 300 + i)
    before = tun.engine.stats()
    assert tun.engine.pkt_launch(False, [], np.zeros(1, np.int32)) == L.OK  # n == 0
    assert tun.engine.stats() == before


def test_slot_limit(tun):
    """AADs of 0, 1, 13, 16, 17 and 1348 bytes with payloads room - 17 .. room, and the relay's
    AAD-only form, both directions; a seal at the limit writes its tag into bytes 2048..2063."""
    for i, la in enumerate(P.limit_launches()):
        run_case(tun, la, 400 + i)


def test_one_byte_past_the_limit_is_refused(tun):
    """NEB_ERR_INVALID for the whole call, nothing launched, statuses and outputs untouched; so
    for more than 32 requests, a NULL argument and an open shorter than its tag."""
    rng = np.random.default_rng(5)
    before = tun.engine.stats()

    def item(a, ln, open_):
        return Item(0, 1, rng.integers(0, 256, a, dtype=np.uint8), rng.integers(0, 256, ln + (16 if open_ else 0), dtype=np.uint8))

    def refused(open_, items):
        _, st, buf, _ = device_launch(tun, open_, items, expect_rc=L.ERR_INVALID)
        assert (st == -77).all() and (buf == GUARD).all()

    for open_, shapes in P.past_limit_calls():
        refused(open_, [item(a, ln, open_) for a, ln in shapes])
    refused(False, [item(16, 100, False) for _ in range(P.COMB_MAX + 1)])
    st = np.full(2, -77, np.int32)
    one = np.zeros(40, np.uint8)
    assert tun.engine.pkt_launch(False, [(tun.kid[0], 1, one[:16], one[:8], None)], st) == L.ERR_INVALID
    assert tun.engine.pkt_launch(True, [(tun.kid[0], 1, one[:16], one[:15], one[20:])], st) == L.ERR_INVALID
    assert L.lib().neb_engine_pkt_launch(tun.engine.handle, 0, None, 1, st.ctypes.data) == L.ERR_INVALID
    assert L.lib().neb_engine_pkt_launch(None, 0, None, 0, None) == L.ERR_INVALID
    assert (st == -77).all() and not one.any()
    assert tun.engine.stats() == before


def test_forgery_matrix(tun):
    """auth_cases.forgery_case over 32 keys, opened in place in launches of 32: one victim per tag
    bit, the first AAD bit, the last AAD byte, the first and the last ciphertext byte and
    counter + 1. Statuses from the oracle; every victim's output zero over len bytes (an empty
    payload changes no byte), every clean neighbour exact, nothing outside any output touched."""
    f = P.forgery()
    b = f.sealed
    sealed = b.arena.copy()
    assert (tun.oracle.batch(b.alg, 0, b.keys, b.desc, sealed) == 0).all()
    tampered = f.tamper(sealed)
    t = Tunnels(tun.engine, tun.oracle, b.keys, tun.kid, tun.chacha_kid)  # the matrix's own 32 keys
    cs = N.CipherAESGCM.CipherBatch(tun.engine, [b.keys[32 * i:32 * i + 32].tobytes() for i in range(P.FORGE_KEYS)])
    t.kid = [c.key_id for c in cs]
    d = b.desc
    seen = set()
    try:
        for lo, hi in P.forgery_cuts():
            items = []
            for i in range(lo, hi):
                a, s, ln, al = (int(d[k][i]) for k in ("aad_off", "src_off", "len", "aad_len"))
                items.append(Item(int(d["key_id"][i]), int(f.open_desc["counter"][i]), tampered[a:a + al].copy(),
                                  tampered[s:s + ln + 16].copy()))
            st, outs = check_launch(t, True, items, f"forgery {lo}")
            for r, i in enumerate(range(lo, hi)):
                if i in f.victims:
                    assert st[r] == L.STATUS_AUTH_FAILED and not outs[r].any(), (i, f.victims[i])
                    seen.add(f.victims[i])
                else:
                    s, ln = int(d["src_off"][i]), int(d["len"][i])
                    assert st[r] == L.STATUS_OK and np.array_equal(outs[r], b.arena[s:s + ln]), i
    finally:
        for c in cs:
            c.destroy()
    assert seen == set(A.KINDS)


def test_other_statuses_in_a_shared_launch(tun):
    """key_id == max_keys and 0xFFFFFFFF, a slot that holds a ChaCha20-Poly1305 key and an
    exhausted counter, each between clean requests that come out exact; a refused request's output
    is untouched. (An open has no counter limit: the oracle opens that request.)"""
    for open_ in (False, True):
        la = P.status_launch(open_)
        st, _ = run_case(tun, la, 500 + open_)
        assert sorted(np.flatnonzero(st).tolist()) == sorted(P.STATUS_SLOTS if not open_ else P.STATUS_SLOTS[:3])
    # the last counter below the limit still seals
    rng = np.random.default_rng(6)
    it = Item(3, L.REJECT_AFTER_MESSAGES - 1, rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, 64, dtype=np.uint8))
    st, _ = check_launch(tun, False, [it, it], "last counter")
    assert (st == L.STATUS_OK).all()


def test_keys_distinct_and_shared(tun):
    """32 requests on 32 keys (every wave stages its own key's tables) and 32 requests on one key."""
    shapes = [P.SIZE_SHAPES[r % len(P.SIZE_SHAPES)] for r in range(P.COMB_MAX)]
    for open_ in (False, True):
        run_case(tun, P.launch(open_, [P.Req(a, ln, r) for r, (a, ln) in enumerate(shapes)], "32 keys"), 600)
        run_case(tun, P.launch(open_, [P.Req(a, ln, 5) for a, ln in shapes], "one key"), 601)
    # one plaintext under 32 keys: 32 different packets
    rng = np.random.default_rng(7)
    aad, pt = rng.integers(0, 256, 16, dtype=np.uint8), rng.integers(0, 256, 100, dtype=np.uint8)
    _, outs = check_launch(tun, False, [Item(r, 9, aad, pt) for r in range(P.COMB_MAX)], "same packet")
    assert len({o.tobytes() for o in outs}) == P.COMB_MAX


def test_same_launch_again(tun):
    """The same launch twice in a row, seal and open alternating on the reused buffers, without a
    stale launch between: identical results."""
    seal = P.launch(False, [P.Req(t.aad_len, t.len, r) for r, t in enumerate(P.SLOT_TYPES * 4)], "again seal")
    open_ = P.launch(True, [P.Req(t.aad_len, t.len, r, t.forged) for r, t in enumerate(P.SLOT_TYPES * 4)], "again open")
    _, si = make_items(tun, seal, 700)
    _, oi = make_items(tun, open_, 701)
    first = None
    for _ in range(2):
        got = (check_launch(tun, False, si, "again seal", stale=False), check_launch(tun, True, oi, "again open", stale=False))
        flat = [x.tobytes() for st, outs in got for x in [st] + outs]
        assert first is None or flat == first
        first = flat


def test_zz_every_launch_ran_the_combined_kernel(engine):
    """neb_engine_pkt_combined rose by exactly the launches and requests this file made."""
    s = engine.stats()
    assert MADE["launches"] > 0
    assert (s["pkt_combined_launches"] - MADE["base"][0], s["pkt_combined_calls"] - MADE["base"][1]) == \
        (MADE["launches"], MADE["calls"])
