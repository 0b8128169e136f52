"""CPU: the directed receive-coalescer cases (tests/coalesce_edge_cases.py) reach what they claim, and
the three forms agree on them without a GPU: the sequential model (coalesce_ref.py), the model of the
device form's plan (coalesce_plan.py: neighbour links, hypothetical chains, pointer jumping) and the
host form (neb_rx_coalesce_batch_host). These are conditions on the cases, not on any kernel: which
bit decides the order of two chain members, the pointer-jumping round in which the last seed is first
marked (the round count parsed from coalesce.hip), the split of every copy as co_gather_kernel makes
it, and the shape each rule case has in the sequential model. Each condition fails when the cases
that carry it are taken out, and the jumping conditions fail when the model runs one round short."""
import functools

import pytest

import coalesce_cases as K
import coalesce_edge_cases as E
import coalesce_plan as PL
import coalesce_ref as M
from nebula_amd import outside as O

EDGE = E.all_cases()
OTHER = K.named_cases() + [(f"random_{seed}", K.random_batch(seed, 1500), K.BOTH) for seed in (41, 42, 43, 44, 45)]
BY_NAME = {c[0]: c for c in EDGE + OTHER}
assert len(BY_NAME) == len(EDGE) + len(OTHER)


@functools.lru_cache(maxsize=None)
def model(name):
    _, packets, lanes = BY_NAME[name]
    return M.coalesce(packets, lanes)


@functools.lru_cache(maxsize=None)
def planned(name):
    _, packets, lanes = BY_NAME[name]
    return PL.plan(packets, lanes)


def shape(name):
    """[(nseg, len)] of the sequential model's writes."""
    return [(w["nseg"], w["len"]) for w in model(name)[0]]


@pytest.mark.parametrize("name", list(BY_NAME))
def test_forms_agree(name):
    """DESIGN §3.9's neighbour-equivalence argument, checked without a GPU: the plan equals the walk."""
    _, packets, lanes = BY_NAME[name]
    want = model(name)
    got = planned(name)[0]
    assert got[2] == want[2] and got[1] == want[1], "plan: per-packet results"
    assert got[0] == want[0], "plan: writes"
    if name == "rule_tcp_udp_same_tuple" or name == "rule_family_only":  # one hash group per lane
        assert PL.plan(packets, lanes, hash_bits=0)[0] == want
    plain, arena = K.stage_padded(packets)
    before = arena.copy()
    host = O.coalesce_batch_host(plain, arena, lanes, K.default_cap(packets), len(packets))
    assert (arena == before).all(), "the input arena is read-only"
    K.assert_equal_model(want, host, name)


def test_every_case_is_small_and_named_once():
    assert len({c[0] for c in EDGE}) == len(EDGE) >= 60
    assert max(len(c[1]) for c in EDGE) == 4097
    for fam in ("sort", "jump", "gather", "rule"):
        assert E.family(EDGE, fam)
    order = [len(c[1]) for c in E.large_small_large(EDGE)]
    assert sorted(order) == sorted(len(c[1]) for c in EDGE)
    assert all(order[i] >= order[i + 1] for i in range(0, len(order) - 1, 2))  # large, then small
    assert all(order[i] <= order[i + 1] for i in range(1, len(order) - 1, 2))  # small, then large


def test_the_round_count_is_read_from_the_source():
    assert [PL.jump_rounds(n) for n in (1, 2, 3, 4, 5, 1024, 1025)] == [0, 1, 2, 2, 3, 10, 11]
    text = PL._source()
    with pytest.raises(AssertionError):
        PL.jump_rounds(8, text.replace("span < n; span <<= 1", "span < len; span <<= 1"))
    with pytest.raises(AssertionError):
        PL.gather_lanes(text.replace("const uint32_t nb = (L - head) / 16u;", "const uint32_t nb = (L - head) >> 4;"))


# ---- sort conditions ---------------------------------------------------------------------------------
def sort_conditions(names):
    """What is missing of: every bit 0..63 of the counter and of the epoch is the most significant bit
    in which two neighbouring members of one chain differ; a tie inside a chain; a tie between flows."""
    bits = dict(counter=set(), epoch=set())
    tie_in_chain = tie_between = False
    for name in names:
        packets = BY_NAME[name][1]
        writes, pw, _ = model(name)
        for w in writes:
            for i, j in zip(w["members"], w["members"][1:]):
                a, b = packets[i], packets[j]
                assert (a["epoch"], a["counter"], i) < (b["epoch"], b["counter"], j)
                if a["epoch"] != b["epoch"]:
                    bits["epoch"].add((a["epoch"] ^ b["epoch"]).bit_length() - 1)
                elif a["counter"] != b["counter"]:
                    bits["counter"].add((a["counter"] ^ b["counter"]).bit_length() - 1)
                else:
                    tie_in_chain = True
        seen = {}
        for i, p in enumerate(packets):
            k = (p["epoch"], p["counter"])
            if k in seen and pw[seen[k]] != pw[i]:
                tie_between = True
            seen.setdefault(k, i)
    missing = [(f, b) for f in ("counter", "epoch") for b in range(64) if b not in bits[f]]
    return missing + [x for x, ok in (("tie in a chain", tie_in_chain), ("tie between flows", tie_between)) if not ok]


def test_sort_conditions():
    names = [c[0] for c in E.family(EDGE, "sort")]
    assert sort_conditions(names) == []

    def without(part):
        return sort_conditions([n for n in names if part not in n])

    assert ("counter", 40) in without("counter_pow2") and ("epoch", 40) in without("epoch_pow2")
    assert ("epoch", 0) in without("special")
    assert ("counter", 0) in sort_conditions([n for n in names if "pow2" in n])  # (1 and 2 differ in bit 1)
    assert "tie between flows" in sort_conditions([n for n in names if "pairwise" not in n and "special" not in n])
    assert without("sort_tie") == ["tie in a chain"]  # (the special values' three flows tie with each other)
    # every reversed or shuffled power-of-two batch is one chain of exactly 64, in counter order
    for n in names:
        if "pow2" in n:
            (w,) = model(n)[0]
            assert w["nseg"] == 64 and w["members"] != sorted(w["members"])
            assert BY_NAME[n][1][w["first"]]["data"] == K.seg(0, size=100)
    assert shape("sort_tie_whole_flow") == [(40, 4040)] and shape("sort_tie_at_max") == [(10, 1040)]
    assert shape("sort_tie_two_flows_pairwise") == [(20, 2040)] * 2
    # input order decides the tie: the flow from port 1001 comes first in the input, so its slot is first
    assert [(w["first"], w["data"][20:22]) for w in model("sort_tie_two_flows_pairwise")[0]] == \
        [(0, (1001).to_bytes(2, "big")), (1, (1000).to_bytes(2, "big"))]
    assert shape("sort_special_values") == [(64, 6440)] * 3 + [(36, 3640)] * 3  # slots in creation order


# ---- jumping conditions ------------------------------------------------------------------------------
def differs_one_round_short(name):
    _, packets, lanes = BY_NAME[name]
    R = planned(name)[1]["R"]
    return PL.plan(packets, lanes, rounds=R - 1)[0] != model(name)


@pytest.mark.parametrize("n", E.JUMP_N)
@pytest.mark.parametrize("form", ["psh", "udp"])
def test_jumping_needs_every_round(form, n):
    name = f"jump_{form}_{n}"
    diag = planned(name)[1]
    R = diag["R"]
    assert R == (n - 1).bit_length() and diag["run_seeds"] == [n] and len(model(name)[0]) == n
    assert max(diag["first_round"].values()) == R  # some seed is first marked in the last round
    if R == 0:
        assert n == 1  # one packet: no round is launched, and there is none to leave out
    else:
        assert differs_one_round_short(name)


def test_jumping_half_batches():
    n = E.HALF_N
    plus, half = planned("jump_half_plus_one")[1], planned("jump_half")[1]
    assert len(BY_NAME["jump_half"][1]) == len(BY_NAME["jump_half_plus_one"][1]) == n
    assert max(plus["run_seeds"]) == n // 2 + 1 and max(half["run_seeds"]) == n // 2
    assert plus["R"] == half["R"] == 10
    assert max(plus["first_round"].values()) == plus["R"] and differs_one_round_short("jump_half_plus_one")
    assert max(half["first_round"].values()) == half["R"] - 1 and not differs_one_round_short("jump_half")
    for name in ("jump_half", "jump_half_plus_one"):  # the rest: passthrough, skipped, a second short flow
        w, _, st = model(name)
        assert sum(x["lane"] == M.LANE_PT for x in w) > 300 and st.count(M.ST_SKIP) > 100
        assert sorted(planned(name)[1]["run_seeds"])[:1] == [1] and (11, 40 + 11 * 200) in shape(name)


def test_jumping_alternating_run():
    assert planned("jump_alternating_chain_and_psh")[1]["run_seeds"] == [40]
    assert shape("jump_alternating_chain_and_psh") == [(64, 40 + 64 * 50), (1, 90)] * 20


# ---- gather conditions -------------------------------------------------------------------------------
def copies(name):
    """(destination, source, length) of every copy the gather makes, both arenas on a 16-byte boundary."""
    plain, _ = K.stage_padded(BY_NAME[name][1])
    return [(dst, int(plain[i]["off"]) + rel, ln) for i, cp in enumerate(planned(name)[1]["copies"]) if cp
            for rel, dst, ln in [cp]]


def gather_conditions(names):
    lanes = PL.gather_lanes()
    pairs, nbs, tails = set(), set(), set()
    short = aligned_after_head = False
    for name in names:
        for dst, src, ln in copies(name):
            head, nb, aligned, tail = PL.gather_split(dst, src, ln)
            assert head + 16 * nb + tail == ln and 0 <= tail < 16
            if nb >= 1:
                pairs.add((dst & 15, src & 15))
            nbs.add(nb)
            tails.add(tail)
            short |= ln < (16 - (dst & 15)) & 15
            aligned_after_head |= aligned and head != 0 and nb >= 1
    missing = [("pair", d, s) for d in range(16) for s in range(16) if (d, s) not in pairs]
    missing += [("nb", x) for x in (0, 1, lanes, lanes + 1) if x not in nbs]
    missing += [("tail", t) for t in range(16) if t not in tails]
    return missing + [x for x, ok in (("L < head", short), ("aligned source after a head", aligned_after_head))
                      if not ok]


def test_gather_conditions():
    names = [c[0] for c in E.family(EDGE, "gather")]
    assert PL.gather_lanes() == 16
    assert gather_conditions(names) == []
    assert gather_conditions(["gather_tcp4"]) == []  # the v4 TCP sweep alone reaches all of it
    rest = gather_conditions([n for n in names if n != "gather_tcp4"])
    assert rest == [("nb", 17)]  # (the other header lengths reach every pair as well)
    assert any(m[0] == "pair" for m in gather_conditions(["gather_short_last", "gather_verbatim"]))
    for kind, hdr in E.HDR.items():
        # flow a's records at source residue a; member k at destination residue (hdr + k g) mod 16
        packets = BY_NAME[f"gather_{kind}"][1]
        plain, _ = K.stage_padded(packets)
        sizes = E.GATHER_ODD + E.GATHER_EVEN if kind == "tcp4" else E.GATHER_OTHER
        assert len(packets) == 256 * len(sizes)
        cps = planned(f"gather_{kind}")[1]["copies"]
        for i in range(len(packets)):
            g, k, a = sizes[i // 256], i // 16 % 16, i % 16
            assert int(plain[i]["off"]) % 16 == a and cps[i][0] == hdr and cps[i][2] == g
            assert cps[i][1] % 16 == (hdr + k * g) % 16
        assert shape(f"gather_{kind}") == [(16, hdr + 16 * g) for g in sizes for _ in range(16)]
    assert shape("gather_short_last") == [(4, 40 + 120 + t) for t in range(1, 16)] + \
        [(4, 28 + 120 + t) for t in range(1, 16)]
    verb = copies("gather_verbatim")
    assert {s & 15 for d, s, ln in verb if ln == 1} == set(range(16))  # the one-byte parsed record
    assert all(d % 16 == 0 for d, s, ln in verb) and len(verb) == 48
    assert {(s & 15) for d, s, ln in verb if ln >= 70} == set(range(16))  # the single-segment "chains"
    assert [w["nseg"] for w in model("gather_verbatim")[0]] == [1] * 48


# ---- rule conditions ---------------------------------------------------------------------------------
def test_rule_case_shapes():
    """Each rule case has, in the sequential model, the shape it is named for: [(nseg, len)]."""
    T, U = M.LANE_TCP, M.LANE_UDP
    assert shape("rule_tcp_udp_same_tuple") == [(6, 640), (6, 628)]
    assert [w["lane"] for w in model("rule_tcp_udp_same_tuple")[0]] == [T, U]
    a, b = BY_NAME["rule_tcp_udp_same_tuple"][1][:2]
    assert a["data"][12:24] == b["data"][12:24] and (a["data"][9], b["data"][9]) == (M.TCP, M.UDP)  # one 38-byte key
    assert shape("rule_family_only") == [(6, 640), (6, 660)]
    big_t, big_u = 60 + E.BIG, 48 + E.BIG
    assert big_t == 65560 and min(big_t, big_u) > M.BUF_SIZE
    assert shape("rule_oversize_tcp6_before") == [(1, 65560), (2, 260)]
    assert shape("rule_oversize_tcp6_between") == [(2, 260), (1, 65560), (2, 260)]
    assert shape("rule_oversize_tcp6_after") == [(2, 260), (1, 65560)]
    assert shape("rule_oversize_tcp6_psh") == [(2, 260), (1, 65560), (2, 260)]
    assert BY_NAME["rule_oversize_tcp6_psh"][1][2]["data"][40 + 13] & M.PSH
    assert shape("rule_oversize_udp6_before") == [(1, big_u), (2, 248)]
    assert shape("rule_oversize_udp6_between") == [(2, 248), (1, big_u), (2, 248)]
    assert shape("rule_oversize_udp6_after") == [(2, 248), (1, big_u)]
    seg, byt = (64, 40 + 6400), (50, 40 + 65000)
    assert shape("rule_after_segcap_fin") == [seg, (1, 140), (3, 340)]
    assert shape("rule_after_segcap_ack") == [seg, (1, 40), (3, 340)]
    assert shape("rule_after_segcap_unparse") == [seg, (1, 140), (3, 340)]
    assert shape("rule_after_segcap_udp0") == [(64, 28 + 6400), (1, 28), (3, 328)]
    assert shape("rule_after_bytecap_fin") == [byt, (1, 1340), (3, 3940)]
    assert shape("rule_after_bytecap_ack") == [byt, (1, 40), (3, 3940)]
    assert shape("rule_after_bytecap_unparse") == [byt, (1, 1340), (3, 3940)]
    assert shape("rule_after_bytecap_udp0") == [(46, 28 + 46 * 1400), (1, 28), (3, 28 + 4200)]
    for cap in ("segcap", "bytecap"):
        # the pure ACK parts nothing: the segment after it links to the chain's last, so only the cap
        # stands between them; behind a FIN the same segment starts a run
        for nm, after in (("ack", True), ("fin", False)):
            link = planned(f"rule_after_{cap}_{nm}")[1]["link"]
            n = len(link)
            assert [link[i] for i in range(n - 4, n)] == [False, after, True, True]
    assert shape("rule_barrier_in_other_lane") == [(4, 440), (1, 140), (1, 128), (4, 428)]
    assert [w["lane"] for w in model("rule_barrier_in_other_lane")[0]] == [T, T, U, U]
