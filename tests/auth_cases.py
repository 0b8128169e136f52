"""Directed cases for the authenticators (GHASH lane layouts, Poly1305 lane layout, tag compare and
wipe), shared by tests/test_auth_cases.py (CPU: the coverage conditions) and
tests/test_gpu_auth_edges.py (GPU: every kernel path against the oracle).

Block-count sweep. Where a lane sits relative to a packet's AAD blocks, payload blocks and length
block depends on na = ceil(aad_len / 16) and m = ceil(len / 16) modulo the lanes per packet L:
n = na + m + 1 blocks are padded in front by (-n) mod L (GCM), and ChaCha20-Poly1305 shifts them by
phi = (4 - na) mod 16. grid() is every (na, m) with na in 0..17, 63, 64, 65 and m in 0..66, with
byte lengths 16·na - pa and 16·m - pm, pa and pm from PADS by a fixed function, so that every
na > 0 and every m > 0 occurs with a whole and with a partial last block.

Forgery matrix. forgery_case() is one batch in which every second packet is a victim: one per tag
bit, the first AAD bit, the last AAD byte, the first and the last ciphertext byte, and counter + 1
in the descriptor; even victims open in place, odd ones out of place at every byte skew of dst.
"""
from dataclasses import dataclass

import numpy as np

from nebula_amd import _lib as L
from nebula_amd import workload as W

NAS = tuple(range(18)) + (63, 64, 65)
MS = tuple(range(67))
PADS = (0, 1, 8, 15)
LANES = (4, 8, 16, 64)


def byte_lens(na: int, m: int):
    """(aad_len, len) of shape (na, m): the last block whole (pad 0) or 15, 8 or 1 bytes long."""
    pa = PADS[(na + m) % 4]
    pm = PADS[(3 * na + m + m // 4) % 4]
    return (16 * na - pa if na else 0), (16 * m - pm if m else 0)


def grid(nas=NAS, ms=MS):
    """[(na, m, aad_len, len)] over nas × ms."""
    return [(na, m) + byte_lens(na, m) for na in nas for m in ms]


def lane_conditions(shapes, lanes: int):
    """The (condition, residue) pairs that `shapes` ((na, m, ...) tuples) leave uncovered at
    `lanes` lanes per packet: every front padding (-n) mod lanes must occur without AAD, with
    fewer AAD blocks than lanes (the AAD ends inside the first round) and with at least as many
    (whole rounds of AAD). An empty list means covered."""
    seen = {"na=0": set(), "0<na<L": set(), "na>=L": set()}
    for s in shapes:
        na, m = s[0], s[1]
        pad = -(na + m + 1) % lanes
        seen["na=0" if na == 0 else "0<na<L" if na < lanes else "na>=L"].add(pad)
    return [(c, r) for c, got in seen.items() for r in range(lanes) if r not in got]


def chacha_conditions(shapes):
    """The (na mod 16, last lane) pairs `shapes` leave uncovered: every AAD phase
    (phi = (4 - na) mod 16) with every lane (n - 1 + phi) mod 16 that the length block can be on."""
    seen = set()
    for s in shapes:
        na, m = s[0], s[1]
        phi = (4 - na) & 15
        seen.add((na % 16, (na + m + phi) % 16))
    return [(a, t) for a in range(16) for t in range(16) if (a, t) not in seen]


# The mixed-key cases give every shape a key of its own with 16, 7 or 3 packets of it, which the
# scheduler plans as a front chunk (4 lanes per packet), a leftover chunk at 8 lanes or one at 16
# (sched.hpp). The front chunks' grid is a cut of grid() (16 packets per shape) that still meets
# lane_conditions at 4 lanes; the leftover chunks run all of it.
FRONT_GRID = (tuple(range(18)), tuple(range(34)))
PER_KEY = {2: 16, 3: 7, 4: 3}  # lg of the lanes per packet -> packets per key


def mixed_grid(lg: int):
    return grid(*FRONT_GRID) if lg == 2 else grid()


def min_blocks(lg: int) -> int:
    """The fewest blocks n a packet must have for the scheduler to run it at 2^lg lanes: size
    class 0 (n <= 4) runs only at 4 lanes and class 1 (n <= 8) at most at 8 (sched_tail_lg)."""
    return {2: 1, 3: 5, 4: 9}[lg]


def desc_shapes(desc: np.ndarray) -> np.ndarray:
    """(na, m) of every descriptor."""
    return np.stack([(desc["aad_len"].astype(np.int64) + 15) // 16, (desc["len"].astype(np.int64) + 15) // 16], 1)


def planned(desc: np.ndarray, max_keys: int = 8192):
    """(lg, front) of every packet: the lanes per packet (log2) of the chunk the mixed-key
    scheduler plans it into (tools/sched_model.plan) and whether that is a front chunk."""
    import os
    import sys

    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import sched_model

    lg = np.full(len(desc), -1, np.int64)
    front = np.zeros(len(desc), bool)
    for c in sched_model.plan(desc["key_id"], desc["aad_len"], desc["len"], max_keys):
        lg[c.packets] = c.lg
        front[c.packets] = c.kind == "front"
    assert (lg >= 0).all()
    return lg, front


def make_batch(alg: int, aad_len, length, key_id, nkeys: int, seed: int, shuffle: bool = True) -> W.Batch:
    """Packets of the given lengths and keys, in place, random contents and counters below 2^62
    from `seed`; AAD slots on 64-byte and payloads on 16-byte boundaries. The descriptors are in
    a shuffled order, so that one wave mixes round counts."""
    rng = np.random.default_rng(seed)
    aad_len, length, key_id = (np.asarray(x, np.int64) for x in (aad_len, length, key_id))
    n = len(length)
    order = rng.permutation(n) if shuffle else np.arange(n)
    aad_len, length, key_id = aad_len[order], length[order], key_id[order]
    src_rel = (aad_len + 15) // 16 * 16
    size = (src_rel + length + 16 + 63) // 64 * 64
    base = np.r_[0, np.cumsum(size)[:-1]] if n else np.zeros(0, np.int64)
    arena = rng.integers(0, 256, int(size.sum()) + 64, dtype=np.uint8)
    desc = np.zeros(n, L.DESC_DTYPE)
    desc["aad_off"] = base
    desc["src_off"] = desc["dst_off"] = base + src_rel
    desc["counter"] = rng.integers(0, 2**62, n, dtype=np.uint64)
    desc["len"] = length
    desc["aad_len"] = aad_len
    desc["key_id"] = key_id
    keys = rng.integers(0, 256, 32 * nkeys, dtype=np.uint8)
    return W.Batch(alg, keys, np.zeros(nkeys, np.uint32), desc, arena, 0, "auth-edges")


def shapes_batch(alg: int, shapes, per_key: int, seed: int, copies: int = 1, nkeys: int = 0) -> W.Batch:
    """nkeys > 0: `copies` packets of every shape over nkeys keys (packet i on key i mod nkeys).
    nkeys = 0: one key per shape, holding per_key packets of it (fresh contents each)."""
    al = np.array([s[2] for s in shapes], np.int64)
    ln = np.array([s[3] for s in shapes], np.int64)
    if nkeys:
        al, ln = np.tile(al, copies), np.tile(ln, copies)
        return make_batch(alg, al, ln, np.arange(len(al)) % nkeys, nkeys, seed)
    kid = np.repeat(np.arange(len(shapes)), per_key)
    return make_batch(alg, np.repeat(al, per_key), np.repeat(ln, per_key), kid, len(shapes), seed)


# ---- forgery matrix --------------------------------------------------------------------------

FORGE_LENS = (0, 1, 17, 100, 1300)
FORGE_N = 272
FORGE_STRIDE = 3072
FORGE_DST = 1536  # out-of-place destinations: slot + FORGE_DST + skew
KINDS = [f"tag_bit_{b}" for b in range(128)] + ["aad_first_bit", "aad_last_byte", "ct_first_byte",
                                                "ct_last_byte", "counter_plus_1"]


@dataclass
class Forgery:
    sealed: W.Batch        # in place; arena = plaintext (seal it with the oracle)
    open_desc: np.ndarray  # the descriptors to open with: victims' dst and counter changed
    victims: dict          # packet index -> kind (all among the first FORGE_N packets)

    def tamper(self, sealed_arena: np.ndarray) -> np.ndarray:
        """The sealed arena with every victim's flip applied (counter_plus_1 flips nothing)."""
        t = sealed_arena.copy()
        d = self.sealed.desc
        for i, kind in self.victims.items():
            a, s, ln, al = (int(d[f][i]) for f in ("aad_off", "src_off", "len", "aad_len"))
            if kind.startswith("tag_bit_"):
                b = int(kind[8:])
                t[s + ln + b // 8] ^= 1 << (b % 8)
            elif kind == "aad_first_bit":
                t[a] ^= 0x80
            elif kind == "aad_last_byte":
                t[a + al - 1] ^= 0x5A
            elif kind == "ct_first_byte":
                t[s] ^= 0x01
            elif kind == "ct_last_byte":
                t[s + ln - 1] ^= 0x80
        return t

    def open_batch(self) -> W.Batch:
        b = self.sealed
        return W.Batch(b.alg, b.keys, b.remote_index, self.open_desc, b.arena, b.stride, "forgery-open")


def forgery_case(alg: int, key_of, nkeys: int, seed: int, rot: int = 0, filler_lens=()) -> Forgery:
    """FORGE_N packets, packet i of FORGE_LENS[(i + rot) mod 5] bytes with a 16-byte AAD (1348 for
    an empty payload), every odd packet a victim: victim v = i // 2 takes KINDS[v mod len(KINDS)].
    A ciphertext victim that lands on an empty payload (rot != 0 only) flips tag bit 0 instead.
    Even victims open in place, odd ones to slot + FORGE_DST + skew, skew = (v // 2) mod 16. Clean
    filler packets of filler_lens follow the matrix. key_of(lens) -> key index of every packet."""
    lens = [FORGE_LENS[(i + rot) % 5] for i in range(FORGE_N)] + list(filler_lens)
    n = len(lens)
    rng = np.random.default_rng(seed)
    arena = rng.integers(0, 256, n * FORGE_STRIDE, dtype=np.uint8)
    desc = np.zeros(n, L.DESC_DTYPE)
    base = np.arange(n, dtype=np.int64) * FORGE_STRIDE
    ln = np.array(lens, np.int64)
    al = np.where(ln == 0, 1348, 16)
    desc["aad_off"] = base
    desc["src_off"] = desc["dst_off"] = base + (al + 15) // 16 * 16
    desc["counter"] = rng.integers(0, 2**62, n, dtype=np.uint64)
    desc["len"] = ln
    desc["aad_len"] = al
    desc["key_id"] = key_of(ln)
    keys = rng.integers(0, 256, 32 * nkeys, dtype=np.uint8)
    od = desc.copy()
    victims = {}
    for i in range(1, FORGE_N, 2):
        v = i // 2
        kind = KINDS[v % len(KINDS)]
        if kind.startswith("ct_") and lens[i] == 0:
            assert rot != 0
            kind = KINDS[0]
        victims[i] = kind
        if kind == "counter_plus_1":
            od["counter"][i] += 1
        if v % 2:
            od["dst_off"][i] = base[i] + FORGE_DST + (v // 2) % 16
    assert ((al + 15) // 16 * 16 + ln + 16 <= FORGE_DST).all() and FORGE_DST + 15 + ln.max() <= FORGE_STRIDE
    b = W.Batch(alg, keys, np.zeros(nkeys, np.uint32), desc, arena, FORGE_STRIDE, "forgery")
    return Forgery(b, od, victims)


def keys_of_equal_length(per_key: int):
    """(key_of, fill): a key assignment for forgery_case in which every key holds exactly per_key
    packets, all of one payload length, so that the mixed-key scheduler plans each key as one
    chunk shape. fill(rot) -> the clean filler lengths that round every length's packet count up
    to a multiple of per_key."""
    def fill(rot):
        lens = [FORGE_LENS[(i + rot) % 5] for i in range(FORGE_N)]
        return [x for x in FORGE_LENS for _ in range(-lens.count(x) % per_key)]

    def key_of(ln):
        kid = np.zeros(len(ln), np.int64)
        nxt = 0
        for x in FORGE_LENS:
            idx = np.flatnonzero(ln == x)
            assert len(idx) % per_key == 0
            kid[idx] = nxt + np.arange(len(idx)) // per_key
            nxt += len(idx) // per_key
        return kid

    return key_of, fill


def mixed_forgery_case(alg: int, lg: int, rot: int) -> Forgery:
    """The matrix over keys of PER_KEY[lg] packets of one length each (rotation rot of the length
    cycle), filled up with clean packets."""
    key_of, fill = keys_of_equal_length(PER_KEY[lg])
    filler = fill(rot)
    return forgery_case(alg, key_of, (FORGE_N + len(filler)) // PER_KEY[lg], seed=100 * lg + rot, rot=rot,
                        filler_lens=filler)
