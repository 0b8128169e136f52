"""CPU: the block-count sweep and the forgery matrix of tests/auth_cases.py cover what they claim.

These are conditions on the cases, not measurements of any kernel: every front padding
(-n) mod L at every lane width L of the GCM kernels with no AAD, with the AAD ending inside the
first round and with whole rounds of AAD; every ChaCha AAD phase with every last lane; every block
count with a whole and a partial last block; the mixed-key batches planned (tools/sched_model.py)
at the lane widths they are meant for; and the matrix's victims."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import auth_cases as A  # noqa: E402
from nebula_amd import _lib as L  # noqa: E402


def test_grid_size_and_lengths():
    g = A.grid()
    assert len(g) == 21 * 67 == 1407
    for na, m, al, ln in g:
        assert (al + 15) // 16 == na and (ln + 15) // 16 == m
    for na in A.NAS[1:]:
        tails = {al % 16 for a, m, al, ln in g if a == na}
        assert 0 in tails and tails - {0}, na
    for m in A.MS[1:]:
        tails = {ln % 16 for a, mm, al, ln in g if mm == m}
        assert 0 in tails and tails - {0}, m
    assert {al % 16 for _, _, al, _ in g} == {ln % 16 for _, _, _, ln in g} == {0, 1, 8, 15}


@pytest.mark.parametrize("lanes", A.LANES)
def test_lane_conditions(lanes):
    assert A.lane_conditions(A.grid(), lanes) == []
    # the check itself notices a hole
    assert A.lane_conditions([s for s in A.grid() if s[0] != 0], lanes)
    assert A.lane_conditions([s for s in A.grid() if -(s[0] + s[1] + 1) % lanes != 1], lanes)


def test_chacha_conditions():
    assert A.chacha_conditions(A.grid()) == []
    assert A.chacha_conditions([s for s in A.grid() if s[0] != 5])
    # the per-packet cases: the AAD phases they have, with every last lane
    per_packet = A.grid((0, 1, 2, 5, 16, 17))
    missing = A.chacha_conditions(per_packet)
    assert {a for a, _ in missing} == set(range(16)) - {0, 1, 2, 5}
    for lanes in (64,):  # gcm_one_kernel runs 64 lanes per packet
        assert {c for c, _ in A.lane_conditions(per_packet, lanes)} == {"na>=L"}


@pytest.mark.parametrize("lg", [2, 3, 4])
def test_mixed_key_batches_are_planned_at_their_width(lg):
    """One key per shape with 16, 7 or 3 packets of it: the scheduler plans every packet long
    enough for 2^lg lanes at exactly that width (16 as a front chunk), the shorter ones narrower,
    and the packets at that width meet the lane conditions."""
    b = A.shapes_batch(L.ALG_AESGCM, A.mixed_grid(lg), A.PER_KEY[lg], seed=lg)
    assert b.nkeys < 8192
    got, front = A.planned(b.desc)
    shapes = A.desc_shapes(b.desc)
    n = shapes[:, 0] + shapes[:, 1] + 1
    wide = n >= A.min_blocks(lg)
    assert (got[wide] == lg).all() and (got[~wide] < lg).all()
    assert (front[wide] == (lg == 2)).all()
    at = [tuple(s) for s in shapes[got == lg]]
    assert A.lane_conditions(at, 1 << lg) == []


def test_forgery_matrix():
    f = A.forgery_case(L.ALG_AESGCM, lambda ln: np.zeros(len(ln), np.int64), 1, seed=1)
    d, od = f.sealed.desc, f.open_desc
    assert len(d) == 272 and sorted(f.victims) == list(range(1, 272, 2))
    assert [int(x) for x in d["len"][:10]] == [0, 1, 17, 100, 1300] * 2
    assert ((d["aad_len"] == 1348) == (d["len"] == 0)).all() and set(d["aad_len"]) == {16, 1348}
    kinds = list(f.victims.values())
    assert set(kinds) == set(A.KINDS) and len(A.KINDS) == 133
    for i, k in f.victims.items():
        if k.startswith("ct_"):
            assert d["len"][i] > 0
    # every payload length among the tag-bit victims of every tag word
    for w in range(4):
        assert {int(d["len"][i]) for i, k in f.victims.items()
                if k.startswith("tag_bit_") and int(k[8:]) // 32 == w} == set(A.FORGE_LENS)
    oop = od["dst_off"] != od["src_off"]
    assert sorted(np.flatnonzero(oop)) == [i for i in f.victims if (i // 2) % 2]
    assert {int(x) % 16 for x in od["dst_off"][oop]} == set(range(16))
    assert (od["src_off"] % 16 == 0).all() and (d["dst_off"] == d["src_off"]).all()
    assert [i for i in range(272) if od["counter"][i] != d["counter"][i]] == \
        [i for i, k in f.victims.items() if k == "counter_plus_1"]
    # the flips: one bit or byte per victim, none for counter_plus_1
    z = np.zeros_like(f.sealed.arena)
    t = f.tamper(z)
    for i in range(272):
        changed = np.flatnonzero(t[i * A.FORGE_STRIDE:(i + 1) * A.FORGE_STRIDE])
        assert len(changed) == (1 if i in f.victims and f.victims[i] != "counter_plus_1" else 0)


@pytest.mark.parametrize("lg", [2, 3, 4])
def test_forgery_matrix_mixed_key_widths(lg):
    """Keys of 16, 7 or 3 packets of one length, over the five rotations of the length cycle:
    every victim kind is planned at 2^lg lanes in some rotation, with payloads to wipe."""
    kinds, wiped = set(), set()
    for rot in range(5):
        f = A.mixed_forgery_case(L.ALG_AESGCM, lg, rot)
        got, _ = A.planned(f.sealed.desc)
        n = A.desc_shapes(f.sealed.desc).sum(axis=1) + 1
        assert (got[n >= A.min_blocks(lg)] == lg).all()
        kinds |= {k for i, k in f.victims.items() if got[i] == lg}
        wiped |= {int(f.sealed.desc["len"][i]) for i in f.victims if got[i] == lg}
    assert kinds == set(A.KINDS)
    assert wiped >= {0, 100, 1300}
