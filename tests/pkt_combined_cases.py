"""Directed cases for the combined per-packet launch (aes_gcm.hip gcm_one_batch_kernel behind
neb_engine_pkt_launch: request r of a launch rides in slot r, one request per wave, four waves per
workgroup), shared by tests/test_pkt_combined_cases.py (CPU: the coverage conditions) and
tests/test_gpu_pkt_combined.py (GPU: every case against the oracle).

A slot holds AAD | payload (+ tag) with the payload at pay = aad_len rounded up to 16. A request
fits when pay + in_len <= 2048 and pay + max(in_len, len + 16) <= 2112 (in_len = len for a seal,
len + 16 for an open), so the largest payload is room = 2048 - pay for a seal (its tag lands in
bytes 2048..2063 of the slot) and 2032 - pay for an open.
"""
from dataclasses import dataclass

import auth_cases as A

COMB_MAX = 32       # requests per launch (cipher.hpp kCombMax)
SLOT = 2112         # bytes per slot (kCombSlot)
ONE_BYTES = 2048    # AAD (padded) + input (kOneBytes)
WAVES = 4           # requests per workgroup (aes_gcm.hip kOneBatchWaves)
ROOM = -1           # a Req's len: the largest payload that fits its AAD and direction

SWEEP_NAS = (0, 1, 2, 5, 16, 17)
SIZES = (1, 2, 3, 4, 5, 31, 32)
LIMIT_AADS = (0, 1, 13, 16, 17, 1348)
RELAY_AAD = 1348  # the relay's AAD-only form: 1348 bytes authenticated, nothing encrypted
STATUS_KINDS = ("key_max_keys", "key_all_ones", "key_chacha_slot", "exhausted")
STATUS_SLOTS = (1, 6, 8, 15)  # wave positions 1, 2, 0, 3


def pay(aad_len: int) -> int:
    return (aad_len + 15) // 16 * 16


def room(open_: bool, aad_len: int) -> int:
    return ONE_BYTES - pay(aad_len) - (16 if open_ else 0)


def fits(open_: bool, aad_len: int, ln: int) -> bool:
    """The engine's rule for a request it combines (comb_core.hpp comb_fits)."""
    in_len = ln + (16 if open_ else 0)
    return pay(aad_len) + in_len <= ONE_BYTES and pay(aad_len) + max(in_len, ln + 16) <= SLOT


@dataclass(frozen=True)
class Req:
    aad_len: int
    len: int
    key: int = 0      # index among the launch's installed keys
    forged: str = ""  # an open launch only: one of auth_cases.KINDS ("" = clean)
    special: str = ""  # one of STATUS_KINDS ("" = none)


@dataclass
class Launch:
    open: bool
    reqs: list
    name: str = ""


def _sized(open_: bool, r: Req) -> Req:
    return Req(r.aad_len, room(open_, r.aad_len), r.key, r.forged, r.special) if r.len == ROOM else r


def launch(open_: bool, reqs, name="") -> Launch:
    reqs = [_sized(open_, r) for r in reqs]
    assert 0 < len(reqs) <= COMB_MAX and all(fits(open_, r.aad_len, r.len) for r in reqs), name
    return Launch(open_, reqs, name)


def chunks(xs, n=COMB_MAX):
    return [xs[i:i + n] for i in range(0, len(xs), n)]


# ---- block-count sweep ---------------------------------------------------------------------------

def sweep_shapes():
    """The 402 shapes the one-packet kernels run (auth_cases.grid over SWEEP_NAS)."""
    return A.grid(SWEEP_NAS)


def sweep_launches(open_: bool):
    return [launch(open_, [Req(al, ln, r) for r, (_, _, al, ln) in enumerate(c)], f"sweep {i}")
            for i, c in enumerate(chunks(sweep_shapes()))]


# ---- slot coverage -------------------------------------------------------------------------------

# Launch j of a direction puts type (r + j) mod 8 into slot r, so over the 8 launches every slot
# holds every type, and every window of 4 consecutive types (a workgroup) has a forged one.
SLOT_TYPES = (
    Req(0, 100),                            # no AAD, a partial last block
    Req(13, 0),                             # an AAD that is no multiple of 16, an empty payload
    Req(17, ROOM),                          # at the slot limit behind an odd AAD
    Req(16, 33, forged="tag_bit_0"),
    Req(RELAY_AAD, 0, forged="aad_last_byte"),  # a forged request with nothing to zero
    Req(0, ROOM),                           # at the slot limit, no AAD
    Req(1, 16),
    Req(16, 1300, forged="ct_last_byte"),
)
SLOT_CONDITIONS = ("no_aad", "odd_aad", "empty", "partial", "seal_limit", "open_limit", "forged", "clean_by_forged")


def slot_cover_launches(types=SLOT_TYPES):
    out = []
    for open_ in (False, True):
        for j in range(len(types)):
            reqs = []
            for r in range(COMB_MAX):
                t = types[(r + j) % len(types)]
                reqs.append(Req(t.aad_len, t.len, r, t.forged if open_ else ""))
            out.append(launch(open_, reqs, f"slots {'open' if open_ else 'seal'} {j}"))
    return out


def slot_conditions(launches):
    """The (condition, slot) pairs `launches` leave uncovered: every slot 0..31, and so every wave
    position r mod 4 of every workgroup, must hold somewhere a request without AAD, one whose AAD
    is no multiple of 16, an empty payload, a payload with a partial last block, a seal and an open
    at the slot limit, a forged request, and a clean request in a workgroup (slots 4g..4g+3 of the
    same launch) that also holds a forged one. An empty list means covered."""
    seen = {c: set() for c in SLOT_CONDITIONS}
    for la in launches:
        for r, q in enumerate(la.reqs):
            if q.special:
                continue
            if q.aad_len == 0:
                seen["no_aad"].add(r)
            if q.aad_len % 16:
                seen["odd_aad"].add(r)
            if q.len == 0:
                seen["empty"].add(r)
            if q.len % 16:
                seen["partial"].add(r)
            if q.len == room(la.open, q.aad_len):
                seen["open_limit" if la.open else "seal_limit"].add(r)
            if la.open and q.forged:
                seen["forged"].add(r)
            group = la.reqs[r // WAVES * WAVES:r // WAVES * WAVES + WAVES]
            if la.open and not q.forged and any(g.forged for g in group):
                seen["clean_by_forged"].add(r)
    return [(c, r) for c in SLOT_CONDITIONS for r in range(COMB_MAX) if r not in seen[c]]


# ---- launch sizes --------------------------------------------------------------------------------

SIZE_SHAPES = ((16, 100), (0, 0), (13, 1300), (0, 17), (48, 16), (1, 1), (RELAY_AAD, 0), (17, 576))


def size_launches():
    return [launch(open_, [Req(*SIZE_SHAPES[r % len(SIZE_SHAPES)], key=r) for r in range(n)], f"n={n}")
            for open_ in (False, True) for n in SIZES]


# ---- the slot limit ------------------------------------------------------------------------------

def limit_requests(open_: bool):
    """(aad_len, len): every LIMIT_AADS with payloads room - 17 .. room, and the relay's AAD-only form."""
    return [(a, ln) for a in LIMIT_AADS for ln in range(room(open_, a) - 17, room(open_, a) + 1)] + [(RELAY_AAD, 0)]


def limit_launches():
    return [launch(open_, [Req(a, ln, r) for r, (a, ln) in enumerate(c)], f"limit {'open' if open_ else 'seal'} {i}")
            for open_ in (False, True) for i, c in enumerate(chunks(limit_requests(open_)))]


def past_limit_calls():
    """[(open, [(aad_len, len)] * 3)]: a request one byte past the limit between two that fit."""
    return [(open_, [(16, 100), (a, room(open_, a) + 1), (0, 0)]) for open_ in (False, True) for a in LIMIT_AADS]


# ---- forgery matrix ------------------------------------------------------------------------------

FORGE_KEYS = 32


def forgery():
    """auth_cases.forgery_case over 32 keys (packet i on key i mod 32), cut into launches of 32."""
    import numpy as np

    from nebula_amd import _lib as L

    return A.forgery_case(L.ALG_AESGCM, lambda ln: np.arange(len(ln)) % FORGE_KEYS, FORGE_KEYS, seed=3200)


def forgery_cuts():
    return [(lo, min(lo + COMB_MAX, A.FORGE_N)) for lo in range(0, A.FORGE_N, COMB_MAX)]


# ---- other statuses inside a shared launch -------------------------------------------------------

def status_launch(open_: bool) -> Launch:
    """Every STATUS_KINDS request between clean ones, the four in four different wave positions."""
    reqs = [Req(16, 100 + r, r) for r in range(17)]
    for slot, kind in zip(STATUS_SLOTS, STATUS_KINDS):
        reqs[slot] = Req(13, 33, slot, special=kind)
    return launch(open_, reqs, f"statuses {'open' if open_ else 'seal'}")
