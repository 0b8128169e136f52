"""CPU: the case set of the TX resolve (tests/tx_resolve_cases.py) holds everything the host and
GPU tests rely on — a missing case fails here rather than going unnoticed — and the model's ECMP
hash (tests/tx_resolve_ref.py) meets the reference's own balance conditions."""
import tx_resolve_cases as TC
import tx_resolve_ref as M
from nebula_amd.hostmap import TxTable

REQUIRED = """v4_len0 v4_len1 v4_len19 v4_len20 v4_ihl_lt20 v4_ihl24_p3 v4_ihl24_p4 v4_icmp_p5 v4_icmp_p6
v4_frag_exact_ihl v4_mf_first v5 v6_len39 v6_len40 v6_hop v6_rt v6_dst v6_ah v6_frag_first v6_frag_later v6_chain8
v6_ext_past v6_echo_p5 v6_echo_p6 v6_nonecho_p3 v6_nonecho_p4 dst_in_net_hit dst_in_net_miss_under_route dst_self4
dst_self6 dst_bcast24 dst_bcast32 dst_mc4 dst_mc6 dst_mc4in6 dst_mapped_of_host route_8 route_16 route_32_and_host
route_default_gw_down route6_32 route6_64 route6_128_gw4 route6_none ecmp_all_down shape_trio2 shape_wrap1
shape_tombstoned shape_behind_tombstone last""".split()


def _results(case):
    return {name: case.model.resolve(bytes(p)) for name, p in case.items}


def _fw(r):
    fw = r[2]
    return {"lport": int.from_bytes(fw[32:34], "little"), "rport": int.from_bytes(fw[34:36], "little"), "proto": fw[36],
            "family": fw[37], "flags": fw[38], "ip_hdr_len": int.from_bytes(fw[40:42], "little"),
            "gateway": int.from_bytes(fw[44:48], "little")}


def test_every_listed_case_is_built():
    case = TC.build()
    assert len(set(case.names)) == len(case.names)
    assert not [n for n in REQUIRED if n not in case.names]
    res = _results(case)
    assert {r[1] for r in res.values()} == {M.OK, M.INVALID, M.TX_DROPPED, M.NO_ROUTE, M.NO_TUNNEL}
    seen = 0
    for r in res.values():
        seen |= r[2][38]
    assert seen == 0x7F  # every NEB_FW_* flag
    st = lambda n: res[n][1]  # noqa: E731
    for n in ("v4_len0", "v4_len1", "v4_len19", "v4_len20", "v4_ihl_lt20", "v4_ihl24_p3", "v4_icmp_p5", "v5", "v6_len39",
              "v6_ext_past", "v6_echo_p5", "v6_nonecho_p3", "v6_frag_short", "v6_udp_p3", "dst_invalid_self"):
        assert st(n) == M.INVALID, n
    for n in ("v4_ihl24_p4", "v4_icmp_p6", "v4_frag_exact_ihl", "v4_mf_first", "v6_len40", "v6_hop", "v6_rt", "v6_dst", "v6_ah",
              "v6_frag_first", "v6_frag_later", "v6_chain8", "v6_echo_p6", "v6_nonecho_p4", "last"):
        assert st(n) == M.OK, n
    # what newPacket leaves behind on an error, and the echo identifier rules
    assert _fw(res["v4_ihl24_p3"])["ip_hdr_len"] == 24 and res["v4_ihl24_p3"][2][:32] == bytes(32)
    assert _fw(res["v4_ihl_lt20"])["ip_hdr_len"] == 0
    assert _fw(res["v6_frag_short"])["flags"] == 0 and _fw(res["v6_echo_p5"])["ip_hdr_len"] == 40
    assert _fw(res["v4_icmp_p6"])["rport"] == 0xBEEF and _fw(res["v4_icmp_p6"])["lport"] == 0
    assert _fw(res["v6_echo_p6"])["rport"] == 0xCAFE and _fw(res["v6_nonecho_p4"])["rport"] == 0
    assert _fw(res["v4_mf_first"])["flags"] == M.FRAG_ANY and _fw(res["v4_mf_first"])["lport"] == 1000
    assert _fw(res["v4_frag_exact_ihl"])["flags"] == M.FRAGMENT | M.FRAG_ANY and _fw(res["v4_frag_exact_ihl"])["rport"] == 0
    assert _fw(res["v6_frag_later"])["flags"] == M.FRAGMENT | M.FRAG_ANY and _fw(res["v6_frag_later"])["ip_hdr_len"] == 48
    assert _fw(res["v6_frag_first"])["flags"] == M.FRAG_ANY and _fw(res["v6_frag_first"])["rport"] == 2000
    assert _fw(res["v6_chain8"])["proto"] == 60 and _fw(res["v6_chain8"])["ip_hdr_len"] == 108  # the ninth header
    assert _fw(res["v6_ah"])["proto"] == M.TCP and _fw(res["v6_ah"])["ip_hdr_len"] == 52
    # gates, in the reference's order
    assert _fw(res["dst_bcast24"])["flags"] == M.GATE_BROADCAST and _fw(res["dst_bcast32"])["flags"] == M.GATE_BROADCAST
    assert _fw(res["dst_self4"])["flags"] == M.GATE_SELF and _fw(res["dst_self6"])["flags"] == M.GATE_SELF
    for n in ("dst_mc4", "dst_mc6", "dst_mc4in6"):
        assert _fw(res[n])["flags"] == M.GATE_MULTICAST and st(n) == M.TX_DROPPED
    # lookups
    assert res["dst_in_net_hit"][:2] == (2, M.OK) and _fw(res["dst_in_net_hit"])["gateway"] == M.GATEWAY_NONE
    assert st("dst_in_net_miss_under_route") == M.NO_TUNNEL and _fw(res["dst_in_net_miss_under_route"])["flags"] == 0
    assert st("dst_mapped_of_host") == M.NO_ROUTE and _fw(res["dst_mapped_of_host"])["family"] == 6
    assert res["route_8"][0] == 4 and res["route_16"][0] == 5 and res["route6_32"][0] == 10 and res["route6_64"][0] == 11
    assert res["route6_128_gw4"][0] == 5 and res["route_32_and_host"][0] == 4 and res["route_gw_is_that_host"][0] == 9
    assert st("route_default_gw_down") == M.NO_TUNNEL and _fw(res["route_default_gw_down"])["gateway"] == 10
    assert st("route6_none") == M.NO_ROUTE
    assert st("ecmp_all_down") == M.NO_TUNNEL and _fw(res["ecmp_all_down"])["flags"] == M.ROUTED
    # ECMP: each bound and the bound plus one choose neighbouring gateways
    first3, first105 = 2, 5  # flat gateway indexes of the two routes in ROUTES_A
    for k in range(3):
        assert _fw(res[f"ecmp111_bound{k}_plus0_0"])["gateway"] == first3 + k
        if k < 2:
            assert _fw(res[f"ecmp111_bound{k}_plus1_1"])["gateway"] == first3 + k + 1
    assert _fw(res["ecmp105_bound0_plus0_0"])["gateway"] == first105 and _fw(res["ecmp105_bound0_plus1_0"])["gateway"] == first105 + 1
    got = {(n.split("_")[0], _fw(r)["gateway"]): (r[0], r[1], _fw(r)["flags"] & M.ECMP_FALLBACK) for n, r in res.items()
           if n.startswith("ecmp1")}
    assert got[("ecmp111", first3)] == (6, M.OK, 0)  # the chosen gateway is up
    assert got[("ecmp111", first3 + 1)] == (6, M.OK, M.ECMP_FALLBACK)  # down, an earlier one is up
    assert got[("ecmp105", first105)] == (8, M.OK, M.ECMP_FALLBACK)  # down, a later one is up
    assert got[("ecmp105", first105 + 1)] == (8, M.OK, 0)
    # layout
    offs = [o for o, _ in case.packets]
    assert {o % 4 for o in offs} == {0, 1, 2, 3} and any(o % 16 == 0 for o in offs)
    assert case.packets[-1][0] + case.packets[-1][1] == len(case.arena) and case.packets[-1][1] > 0


def test_table_shapes():
    case = TC.build()
    with TxTable(None, TC.HOSTS, TC.ROUTES, TC.GATEWAYS) as t:
        TC.load(t, case)
        trio = [t.probe(a) for a in case.trio]
        assert [p[0] for p in trio] == [True] * 3 and [p[2] for p in trio] == [1, 2, 3]
        w0, w1 = (t.probe(a) for a in case.wrap)
        assert w0 == (True, TC.SLOTS - 1, 1) and w1[0] and w1[1] < w0[1] and w1[2] >= 2  # the chain wraps
        gone, behind = (t.probe(a) for a in case.pair)
        assert not gone[0] and behind[0] and behind[2] == 2 and gone[2] == 3  # a tombstone in front
        assert t.probe("198.51.100.5")[0] and t.probe("198.51.100.5/32", route=True)[0]  # one address, both kinds
        assert not t.probe("198.51.100.5/31", route=True)[0]
        assert t.count() == (len(case.model.hosts), len(TC.ROUTES_A))


def test_model_hash_balances_as_the_reference_requires():
    """routing/balance_test.go:54-57 and :101-102: over the port pairs (i, 65535 - i) each of three
    equal gateways gets 65535/3 within 100, and weights 10:5 get 2/3 and 1/3 within 100."""
    assert M.buckets([1, 1, 1]) == [715827882, 1431655764, 2147483647]
    for weights in ((1, 1, 1), (10, 5)):
        bounds = M.buckets(weights)
        counts = [0] * len(weights)
        for i in range(65535):
            counts[M.balance(M.hash_packet(i, 65535 - i), bounds)] += 1
        for c, w in zip(counts, weights):
            assert abs(c - 65535 * w / sum(weights)) <= 100, counts
