"""CPU: the directed batches of tests/rx_report_cases.py really reach the conditions they are named
for, judged on the model (tests/rx_report_ref.py) alone: no library call here."""
import numpy as np
import pytest

import rx_report_cases as RC
import rx_report_ref as M
from nebula_amd import _lib as L

CASES = {c.name: c for c in RC.directed()}
_WANT = {}


def want(name):
    if name not in _WANT:
        _WANT[name] = M.report(CASES[name].batch)
    return _WANT[name]


def walked(name):
    cp = CASES[name].plane()
    M.walk(CASES[name].batch, cp)
    return cp


def packets(name):
    b = CASES[name].batch
    return [M.packet(b, i) for i in range(len(b))]


def test_case_names_are_unique():
    assert len(CASES) == len(RC.directed())


@pytest.mark.parametrize("name", ["matrix", "matrix_relayed", "matrix_per_packet_from", "matrix_no_from"])
def test_matrix_holds_every_status_with_every_header(name):
    seen = {(p.status, p.type, p.sub, p.ver, p.key_id == L.KEYS_MIXED) for p in packets(name)}
    for st in RC.ALL_STATUS:
        for t in range(8):
            for s in range(3):
                for v in (1, 2):
                    assert (st, t, s, v, False) in seen and (st, t, s, v, True) in seen
    assert {L.STATUS_OK, L.STATUS_AUTH_FAILED, L.STATUS_BAD_KEY, L.STATUS_REPLAY, L.STATUS_INVALID, L.STATUS_NOT_MESSAGE,
            L.STATUS_NOT_RELAYED} <= set(RC.ALL_STATUS)
    assert any(not M.valid_subtype(p.type, p.sub) for p in packets(name))
    w = want(name)
    # every metric slot that is counted is reached, and every kind of work but what the mode excludes
    assert all(w.metrics[k] > 0 for k in range(L.METRIC_NO_TUNNEL + 1)), w.metrics
    assert (w.metrics[L.METRIC_NO_TUNNEL + 1:] == 0).all()
    kinds = set(w.work["kind"].tolist())
    relayed = CASES[name].batch.relayed
    every = set(range(L.WORK_HANDSHAKE, L.WORK_CONTROL + 1))
    assert kinds == every - ({L.WORK_SEND_RECV_ERROR} if relayed else {L.WORK_NESTED_RELAY})
    # TestReply opens and is not listed
    listed = set(w.work["packet"].tolist())
    replies = [p for p in packets(name) if p.status == L.STATUS_OK and p.type == M.TEST and p.sub == 1]
    assert replies and not any(p.i in listed for p in replies)
    assert w.counts[2] == 3  # the three relay indexes of authenticated Message/Relay packets


def test_matrix_sources_by_mode():
    assert want("matrix").counts[0] > want("matrix_no_from").counts[0] == want("matrix_relayed").counts[0] == 2
    assert (want("matrix_no_from").runs["from"]["family"] == 0).all()
    assert (want("matrix_relayed").runs["from"]["family"] == 0).all()
    assert want("matrix").runs.tobytes() == want("matrix_per_packet_from").runs.tobytes()
    assert {0, 4} <= set(want("matrix").runs["from"]["family"].tolist())


def test_own_source_counts_no_rx_unless_relayed():
    plain, own, own_rel, rel = (want(n).metrics for n in ("matrix", "own_source", "own_source_relayed", "matrix_relayed"))
    assert all(p.own for p in packets("own_source"))
    assert (own[:L.METRIC_RX_INVALID] == 0).all() and (plain[:L.METRIC_RX_INVALID] > 0).all()
    assert own_rel[:L.METRIC_RX_INVALID].tolist() == rel[:L.METRIC_RX_INVALID].tolist() == plain[:L.METRIC_RX_INVALID].tolist()
    assert own[L.METRIC_RX_INVALID] == plain[L.METRIC_RX_INVALID]  # by status alone


@pytest.mark.parametrize("name", ["lens", "lens_relayed"])
def test_lens(name):
    ps = packets(name)
    assert {p.len for p in ps} == {0, 1, 2, 15, 16, 31, 32}
    for ln in (0, 1, 2, 15, 16, 31, 32):
        assert {p.status for p in ps if p.len == ln} == set(RC.ALL_STATUS)
    w = want(name)
    # rx.invalid: lengths 2, 15, 16, 31, 32 of the INVALID packets; 0 and 1 are hole punches
    inv = [p for p in ps if p.status == L.STATUS_INVALID]
    assert w.metrics[L.METRIC_RX_INVALID] == sum(p.len > 1 for p in inv) == len(inv) * 5 // 7
    # nothing shorter than a header is listed, and nothing of it counts an Rx
    listed = set(w.work["packet"].tolist())
    assert listed and all(ps[i].len >= 16 for i in listed)
    short = [p for p in ps if p.len < 16]
    rx = sum(int(w.metrics[k]) for k in range(L.METRIC_RX_INVALID))
    assert rx == sum(1 for p in ps if p.len >= 16 and p.type != M.MESSAGE) and short
    # a short opened packet still enters its run with its length
    assert w.metrics[L.METRIC_OPENED_BYTES] == sum(p.len for p in ps if p.status == L.STATUS_OK)
    assert w.counts[2] == 1  # relay packets of 16, 31 and 32 bytes, one index


def test_padding_and_entry_out_of_range():
    b, w = CASES["padding_and_entry_out_of_range"].batch, want("padding_and_entry_out_of_range")
    assert L.RECV_NONE in b.pkt_entry.tolist() and any(L.RECV_NONE != e >= len(b.frm) for e in b.pkt_entry.tolist())
    assert len(b.frm) == 1
    assert [(int(r["packet"]), int(r["packets"]), int(r["from"]["family"])) for r in w.runs] == [(0, 1, 4), (2, 3, 0), (5, 1, 4)]
    assert w.work.tolist() == [(6, L.WORK_SEND_RECV_ERROR)]
    assert w.metrics[L.METRIC_RX_INVALID] == 0  # padding is not counted
    cp = walked("padding_and_entry_out_of_range")
    assert cp.roams == 1


def test_roaming_sequences():
    fam = lambda w: [r["from"].tobytes() for r in w.runs]  # noqa: E731
    w = want("roam_AABAR_allowed")
    assert fam(w) == [RC.A, RC.B, RC.A, RC.R] and w.runs["packets"].tolist() == [2, 1, 1, 1]
    cp = walked("roam_AABAR_allowed")
    # A taken, B taken, back to A suppressed (the clock is frozen), R taken
    assert (cp.roams, cp.suppressed, cp.denied) == (3, 1, 0) and cp.remote[7] == RC.R
    cp = walked("roam_AABAR_A_denied")
    # A refused three times, B taken, and R, where the tunnel just came from, suppressed
    assert (cp.roams, cp.denied, cp.suppressed) == (1, 3, 1) and cp.remote[7] == RC.B and cp.last_roam_remote[7] == RC.R
    cp = walked("roam_back_suppressed")
    assert cp.suppressed == 2 and cp.roams == 2 and cp.remote[7] == RC.A and cp.last_roam_remote[7] == RC.R
    cp = walked("roam_back_after_suppression")
    # the old suppression has run out, so A is taken; the way back to B is then suppressed in turn
    assert cp.suppressed == 1 and cp.roams == 1 and cp.remote[7] == RC.A and cp.last_roam[7] == cp.now


@pytest.mark.parametrize("name, what", [("sources_differ_in_port", "port"), ("sources_differ_in_family", "family"),
                                        ("sources_differ_in_last_address_byte", "addr")])
def test_sources_that_differ_in_one_field(name, what):
    w = want(name)
    assert w.counts[0] == len(CASES[name].batch) and w.counts[1] == 1
    a, b = w.runs["from"][0], w.runs["from"][1]
    for f in ("port", "family", "addr"):
        assert (a[f].tobytes() != b[f].tobytes()) == (f == what), f
    if what == "addr":
        assert [i for i in range(16) if a["addr"][i] != b["addr"][i]] == [15]
        assert [i for i in range(16) if w.runs["from"][2]["addr"][i] != w.runs["from"][3]["addr"][i]] == [15]


def test_tunnel_shapes():
    assert want("one_tunnel_all_packets").counts.tolist() == [1, 1, 0, 0]
    assert want("one_tunnel_all_packets").runs["packets"].tolist() == [600]
    w = want("every_packet_its_own_tunnel")
    assert w.counts.tolist() == [600, 600, 0, 0] and w.runs["key_id"].tolist() == list(range(600))
    assert w.runs["packet"].tolist() != sorted(w.runs["packet"].tolist())  # arrival order is not key order
    w = want("key_ids_differ_in_a_high_bit")
    keys = w.runs["key_id"].tolist()
    assert keys == sorted(keys) and len(keys) == 7 and L.KEYS_MIXED in keys
    assert any(a ^ b == 1 << 31 for a in keys for b in keys) and (w.runs["packets"] == 10).all()
    w = want("relay_tunnel_64_interleaved_indexes")
    assert w.counts.tolist() == [1, 1, 64, 0] and (w.relay_used["packets"] == 10).all()
    idx = w.relay_used["index"].tolist()
    assert idx == sorted(idx) and max(idx) >= 1 << 31


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70000])
def test_sizes(n):
    assert len(CASES[f"n_{n}"].batch) == n
    w = want(f"n_{n}")
    assert w.counts[0] >= 1
    if n >= 255:
        assert all(c > 0 for c in w.counts.tolist()) and w.counts[0] > w.counts[1]
    assert len(CASES["empty"].batch) == 0 and want("empty").counts.tolist() == [0, 0, 0, 0]


def test_heads_on_both_sides_of_a_block_edge():
    w = want("run_heads_at_a_block_edge")
    assert w.runs["packet"].tolist() == [0, 255, 256, 257, 511, 512]  # one tunnel, all opened: position = index
    w = want("tunnel_and_relay_heads_at_a_block_edge")
    assert w.runs["packet"].tolist() == [0, 256] and w.relay_used.tolist() == [(1, 256), (2, 344)]


def test_random_batches_cover_the_modes():
    bs = RC.random_batches(77, 12, 300)
    assert {(b.frm is None, b.pkt_entry is None, b.relayed) for b in bs} >= {(True, True, False), (False, False, False),
                                                                            (False, True, False), (False, False, True)}
    assert all(1 <= len(b) <= 300 for b in bs)
    assert isinstance(bs[0].pk, np.ndarray)
