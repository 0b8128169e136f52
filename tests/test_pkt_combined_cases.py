"""CPU: the directed cases of the combined per-packet launch (tests/pkt_combined_cases.py) meet
their coverage conditions, and the conditions notice a case that is missing. The GPU side,
tests/test_gpu_pkt_combined.py, runs exactly these cases against the oracle."""
import auth_cases as A
import pkt_combined_cases as P


def test_fit_rule_and_room():
    for open_ in (False, True):
        for a in P.LIMIT_AADS + (48, 2033):
            rm = P.room(open_, a)
            if rm < 0:
                assert not P.fits(open_, a, 0)
                continue
            assert P.fits(open_, a, rm) and not P.fits(open_, a, rm + 1), (open_, a)
    # a seal at the limit writes its tag into bytes 2048..2063 of the slot
    assert P.pay(17) + P.room(False, 17) == 2048 and 2048 + 16 <= P.SLOT
    assert P.room(False, 0) == 2048 and P.room(True, 0) == 2032 and P.room(True, 1348) == 672


def test_sweep_is_the_one_packet_kernels_grid():
    shapes = P.sweep_shapes()
    assert len(shapes) == 402 and shapes == A.grid((0, 1, 2, 5, 16, 17))
    # at 64 lanes per request: every front padding without AAD and with fewer AAD blocks than lanes
    assert {c for c, _ in A.lane_conditions(shapes, 64)} == {"na>=L"}
    for open_ in (False, True):
        ls = P.sweep_launches(open_)
        assert len(ls) == 13 and sum(len(la.reqs) for la in ls) == 402
        assert [(q.aad_len, q.len) for la in ls for q in la.reqs] == [(s[2], s[3]) for s in shapes]
        assert all(len({q.key for q in la.reqs}) == len(la.reqs) for la in ls)  # a key per slot


def test_slot_coverage():
    ls = P.slot_cover_launches()
    assert P.slot_conditions(ls) == []
    assert all(len(la.reqs) == P.COMB_MAX for la in ls) and len(ls) == 16
    # the conditions notice what is missing: types dropped, one direction only, a slot short
    clean = tuple(t for t in P.SLOT_TYPES if not t.forged)
    assert {c for c, _ in P.slot_conditions(P.slot_cover_launches(clean))} == {"forged", "clean_by_forged"}
    small = tuple(t for t in P.SLOT_TYPES if t.len != P.ROOM)
    assert {c for c, _ in P.slot_conditions(P.slot_cover_launches(small))} >= {"seal_limit", "open_limit"}
    with_aad = tuple(t for t in P.SLOT_TYPES if t.aad_len)
    assert "no_aad" in {c for c, _ in P.slot_conditions(P.slot_cover_launches(with_aad))}
    assert {c for c, _ in P.slot_conditions([la for la in ls if la.open])} == {"seal_limit"}
    assert {c for c, _ in P.slot_conditions([la for la in ls if not la.open])} == {"open_limit", "forged", "clean_by_forged"}
    short = [P.Launch(la.open, la.reqs[:31], la.name) for la in ls]
    assert {r for _, r in P.slot_conditions(short)} == {31}
    # every workgroup of every open launch mixes clean and forged requests
    for la in ls:
        if la.open:
            for g in range(0, 32, P.WAVES):
                kinds = {bool(q.forged) for q in la.reqs[g:g + P.WAVES]}
                assert kinds == {True, False}, (la.name, g)


def test_launch_sizes():
    ls = P.size_launches()
    for open_ in (False, True):
        assert tuple(len(la.reqs) for la in ls if la.open == open_) == (1, 2, 3, 4, 5, 31, 32)
    # idle waves in the last workgroup (n mod 4 = 1, 2, 3), one workgroup, eight
    assert {n % P.WAVES for n in P.SIZES} == {0, 1, 2, 3} and 4 in P.SIZES and 32 in P.SIZES


def test_slot_limit_cases():
    for open_ in (False, True):
        reqs = P.limit_requests(open_)
        for a in (0, 1, 13, 16, 17, 1348):
            rm = (2048 if not open_ else 2032) - P.pay(a)
            assert {ln for x, ln in reqs if x == a and ln} >= set(range(rm - 17, rm + 1)), (open_, a)
        assert (1348, 0) in reqs  # the relay's AAD-only form
        assert all(P.fits(open_, a, ln) for a, ln in reqs)
    ls = P.limit_launches()
    assert sum(len(la.reqs) for la in ls) == 2 * (6 * 18 + 1) and len(ls) == 8
    past = P.past_limit_calls()
    assert {(o, rs[1][0]) for o, rs in past} == {(o, a) for o in (False, True) for a in P.LIMIT_AADS}
    for open_, rs in past:
        assert [P.fits(open_, a, ln) for a, ln in rs] == [True, False, True]
        assert P.fits(open_, rs[1][0], rs[1][1] - 1)


def test_forgery_matrix_cut_into_launches():
    f = P.forgery()
    assert f.sealed.n == A.FORGE_N == 272 and sorted(f.victims) == list(range(1, 272, 2))
    assert set(f.victims.values()) == set(A.KINDS)
    assert set(f.sealed.desc["key_id"]) == set(range(32))
    cuts = P.forgery_cuts()
    assert [hi - lo for lo, hi in cuts] == [32] * 8 + [16] and cuts[0][0] == 0 and cuts[-1][1] == 272
    d = f.sealed.desc
    assert all(P.fits(True, int(d["aad_len"][i]), int(d["len"][i])) for i in range(272))
    # victims in every wave position that an odd packet index can take, empty payloads among them
    assert {i % P.WAVES for i in f.victims} == {1, 3}
    assert any(int(d["len"][i]) == 0 for i in f.victims) and any(int(d["len"][i]) == 1300 for i in f.victims)


def test_status_launch():
    for open_ in (False, True):
        la = P.status_launch(open_)
        special = {r: q.special for r, q in enumerate(la.reqs) if q.special}
        assert tuple(special.values()) == P.STATUS_KINDS
        assert {r % P.WAVES for r in special} == {0, 1, 2, 3}
        for r in special:  # each between clean requests
            assert not la.reqs[r - 1].special and not la.reqs[r + 1].special
