"""CPU: the directed replay-window cases (tests/rxwin_cases.py) reach what they claim. These are
conditions on the cases, not on any kernel: every scripted step with the oracle's outcome at every
length, the window relations the finish kernels branch on (ranges that wrap or straddle a bitmap
word, a clear of exactly len and len - 1 slots, counters admitted and pushed out in one batch beside
old ones, the end of warmup inside a batch), the positions of run heads and carried maxima in the
scan blocks and sort workgroups (geometry parsed from rxwin.hpp / rxwin.hip), what a strict batch
may hold, and the parallel form's model (tools/rxwin_model.py) against the sequential oracle on
every unforged run of every case. Each condition fails when the runs that carry it are taken out."""
import pytest

import replay_oracle as R
import rxwin_cases as C
import rxwin_model as M


@pytest.fixture(scope="module")
def cases():
    return C.cases()


def _family(cases, fam):
    return [c for c in cases.values() if c.family == fam]


def _arith(cases):
    return [c for c in _family(cases, "arith") if c.name.startswith("arith_")]


def test_geometry_is_read_from_the_sources():
    k = C.constants()
    assert k["block"] > 1 and k["sort_blocks"] > 1 and k["sort_threads"] > 1 and k["sort_digit"] > 1
    assert k["risky"] > 1 << 32


def test_every_step_with_the_oracles_outcome(cases):
    ar = _arith(cases)
    assert [c.length for c in ar] == list(C.LENGTHS)
    assert C.step_conditions(ar) == []
    # the check itself notices a hole: no full script, one length gone, the counter-0 steps gone
    short = [C.arith_case(L, [r for r in C.arith_runs(L) if r[1] != "full"]) for L in (2, 64)]
    assert C.step_conditions(short, (2, 64))
    assert {m[0] for m in C.step_conditions([c for c in ar if c.length != 32])} == {32}
    only = [C.arith_case(64, [("n62a", "full")])]  # no room for the jump of 3 len below 2^62
    assert C.step_conditions(only, (64,)) == [(64, "+3len", R.OK)]


def test_window_relations(cases):
    recs = [r for c in _arith(cases) for r in c.replayed()[3]]
    assert C.window_conditions(recs) == []
    # per length: the starts that place a short range on the ring's end or on a word boundary, the
    # scripts that advance by exactly len - 1, the warmup starts
    for L in (2, 16, 128, 65536):
        mine = [r for r in recs if r["length"] == L]

        def missing(keep):
            return {f for _, f in C.window_conditions([r for r in mine if keep(r["label"])], (L,))}

        assert "clear_len-1" in missing(lambda lb: lb[1] != "adv_lm1")
        assert "warmup_crossed" in missing(lambda lb: lb[0] not in ("zero", "lenm1"))
        if L >= 16:
            assert {"clear_wraps", "leave_wraps"} <= missing(lambda lb: lb[1] not in ("small", "adv_lm1"))
        if L >= 128:
            # (a warmup window's leaving range starts at counter 1 and straddles words as well)
            assert {"clear_straddles", "leave_straddles"} <= missing(
                lambda lb: lb[1] not in ("small", "adv_lm1") and lb[0] not in ("zero", "lenm1", "len"))
        assert "both_left" in missing(lambda lb: lb[1] in ("small", "adv_lm1") and lb[0] in ("zero", "lenm1"))


def test_positions_in_scan_blocks_and_sort_workgroups(cases):
    pos = _family(cases, "position")
    assert C.position_conditions(pos) == []
    for kind in C.POSITION_WANT:  # every kind of case carries something
        assert C.position_conditions([x for x in pos if not x.name.startswith(kind)]), kind
    lay = C.layout(cases["pos_lookback"])
    assert lay["n"] == C.BIG_N == 16909 and lay["items"] == 2 and lay["per_blk"] == 512
    assert lay["lens"] == [3, 66 * 256 + 10]
    assert C.layout(cases["pos_heads_1024"])["lens"] == list(C.P1_SIZES)
    # the arrival order is not the run order: the sort has work to do
    for c in pos:
        lay = C.layout(c)
        assert lay["order"] != list(range(lay["n"])), c.name


def test_only_one_case_is_large(cases):
    big = [c.name for c in cases.values() if max(len(b) for b, _ in c.batches) > 3000]
    assert big == ["pos_lookback"]


def test_strict_batches_can_stay_on_the_device(cases):
    for c in cases.values():
        assert C.strict_violations(c) == [], c.name
    assert {c.family for c in cases.values() if not c.strict} == {"carried", "forged"}
    # the check notices each reason
    f = cases["forged_twin"]
    assert C.strict_violations(C.Case("x", "forged", f.length, f.history, [(f.batches[0][0], True)], absent=f.absent))
    L = 64
    risky = C.constants()["risky"]
    assert C.strict_violations(C.Case("y", "arith", L, {0: [5]}, [([(0, risky, False)], True)]))
    assert C.strict_violations(C.Case("z", "arith", L, {0: [risky + 5]}, [([(0, 3, False)], True)]))


def test_carried_state_cases(cases):
    c = cases["carried_twice"]
    st, _, _, recs = c.replayed()
    n = len(c.batches[0][0])
    assert c.batches[0][0] == c.batches[1][0] and R.OK in st[:n] and R.REPLAY in st[:n]
    assert st[n:] == [R.REPLAY] * n
    for r in recs:
        if r["batch"] == 1:  # refused by Check: Update never runs, so nothing of the window moves
            assert (r["cur"], r["bits"], r["lost"]) == (r["cur0"], r["bits0"], r["lost0"])
    c = cases["carried_small_after_large"]
    (b0, _), (b1, _) = c.batches
    assert len(b1) * 4 < len(b0)
    again = [i for i, a in enumerate(b1) if a in b0]
    assert again and all(b0.index(b1[i]) != i for i in again)  # the same keys at other arrival indices
    st = c.replayed()[0][len(b0):]
    assert R.OK in st and R.REPLAY in st
    c = cases["carried_host_then_strict"]
    (b0, s0), (b1, s1) = c.batches
    assert (s0, s1) == (False, True) and [a[0] for a in b0 if a[2]] == [0] and not any(a[2] for a in b1)
    st = c.replayed()[0]
    mask = c.length - 1
    words0 = {(a[1] & mask) >> 6 for a, s in zip(b0, st) if a[0] == 0 and s == R.OK}
    words1 = {(a[1] & mask) >> 6 for a, s in zip(b1, st[len(b0):]) if a[0] == 0 and s == R.OK}
    assert words0 and words1 <= words0 and c.length // 64 > 1


def test_forged_roles(cases):
    for L in (2, 64, 1024):
        c = cases[f"forged_jump_{L}"]
        st = c.replayed()[0]
        forged = [i for i, a in enumerate(c.batches[0][0]) if a[2]]
        assert len(forged) == 3 and all(c.kinds[i] == "+len" and st[i] == R.AUTH_FAILED for i in forged)
        twins = [i for i, k in enumerate(c.kinds) if k == "+len_twin"]
        assert len(twins) == 3 and all(st[i] == R.OK for i in twins)
        for i, j in zip(forged, twins):
            assert c.batches[0][0][i][:2] == c.batches[0][0][j][:2] and i < j
    c = cases["forged_twin"]
    st = c.replayed()[0]
    lay = C.layout(c)
    arr = c.batches[0][0]
    (fi,) = [i for i, a in enumerate(arr) if a[2]]
    pos = {i: p for p, i in enumerate(lay["order"])}
    ti = lay["order"][pos[fi] + 1]
    assert (pos[fi], pos[ti]) == (lay["block"] - 1, lay["block"]) and arr[ti] == (arr[fi][0], arr[fi][1], False)
    assert (st[fi], st[ti]) == (R.AUTH_FAILED, R.OK)
    gone = [i for i, a in enumerate(arr) if a[0] in c.absent]
    assert gone and lay["order"][-len(gone):] == gone and all(st[i] == R.BAD_KEY for i in gone)


def test_model_equals_oracle_on_every_unforged_run(cases):
    """tools/rxwin_model.py (admit, finish_ranges, finish) against the sequential oracle, on these
    inputs: what tests/test_rxwin_model.py checks on random streams."""
    nruns = 0
    for c in cases.values():
        for r in c.replayed()[3]:
            if r["forged"]:
                continue  # the parallel form is for runs whose tags all verify
            L = r["length"]
            adm = M.admit(r["run"], r["cur0"], r["bits0"], L)
            assert adm == [s == R.OK for s in r["status"]], (c.name, r["tunnel"])
            fins = (M.finish_ranges,) if L > 1024 else (M.finish_ranges, M.finish)
            for fin in fins:
                cur, bits, lost = fin(r["run"], adm, r["cur0"], r["bits0"], r["lost0"], L)
                assert (cur, lost) == (r["cur"], r["lost"]), (c.name, r["tunnel"], fin.__name__)
                assert bits == r["bits"], (c.name, r["tunnel"], fin.__name__)
            nruns += 1
    assert nruns > 350


def test_host_window_class_on_every_case(cases):
    """The engine's C++ window (neb_window_*, the class behind the host receive and the device
    windows' load / store), packet by packet as ConnectionState.Decrypt drives it, against the
    oracle on the same histories and arrivals: verdicts, counters and, up to length 1024, bitmaps."""
    from nebula_amd.connection_state import Bits

    for c in cases.values():
        st, _, owins, _ = c.replayed()
        wins = {}
        for t in owins:
            w = Bits(c.length)
            for x in c.history.get(t, []):
                w.Update(x)
            wins[t] = w
        got = []
        for t, ctr, forged in c.arrivals:
            w = wins.get(t)
            if w is None:
                got.append(R.BAD_KEY)
            elif not w.Check(ctr):
                got.append(R.REPLAY)
            elif forged:
                got.append(R.AUTH_FAILED)
            else:
                got.append(R.OK if w.Update(ctr) else R.REPLAY)
        assert got == st, c.name
        for t, w in wins.items():
            o = owins[t]
            assert (w.current, w.lost, w.dupe, w.out_of_window) == (o.current, o.lost, o.dupe, o.out_of_window)
            if c.length <= 1024:
                assert [bool(b) for b in w.snapshot()] == o.snapshot(), (c.name, t)
