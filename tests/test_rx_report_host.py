"""CPU: neb_rx_report_batch_host against the per-packet model (tests/rx_report_ref.py). Every directed
case of tests/rx_report_cases.py and a seeded random set: the five outputs byte for byte with nothing
written past the counts, and the report replayed through the toy control plane ends in the state the
per-packet walk ends in, with the same dispatch log in the same order. Then the argument errors and the
arena check."""
import ctypes as C

import numpy as np
import pytest

import rx_report_cases as RC
import rx_report_ref as M
from nebula_amd import _lib as L
from nebula_amd.outside import report_host

SLACK = 3
DIRECTED = RC.directed()
RANDOM = RC.random_batches(20261, 30, 1500)
_vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731


def run_raw(b: M.Batch, arena_len=None):
    """The host form into FILL-initialised outputs with SLACK records beyond n."""
    n = len(b)
    outs = {name: np.full((n + SLACK) * item, RC.FILL, np.uint8) for name, item in RC.OUT_ITEMS}
    metrics = np.full(L.REPORT_NMETRICS, 0xA5A5A5A5, np.uint64)
    counts = np.full(4, 0xA5A5A5A5, np.uint32)
    rc = L.lib().neb_rx_report_batch_host(_vp(b.pk), _vp(b.status), n, _vp(b.arena), b.arena.nbytes if arena_len is None else arena_len,
                                          _vp(b.frm), _vp(b.pkt_entry), 0 if b.frm is None else len(b.frm),
                                          L.REPORT_RELAYED if b.relayed else 0, _vp(outs["runs"]), _vp(outs["relay_used"]),
                                          _vp(outs["work"]), _vp(metrics), _vp(counts))
    return rc, outs, metrics, counts


def check(b: M.Batch, plane=M.ControlPlane):
    want = M.report(b)
    rc, outs, metrics, counts = run_raw(b)
    assert rc == L.OK
    RC.compare(outs, metrics, counts, want, len(b), SLACK)
    # the report replayed against the packets walked one by one
    r = report_host(b.pk, b.status, b.arena, b.frm, b.pkt_entry, b.relayed)
    by_packet, by_report = plane(), plane()
    M.walk(b, by_packet)
    M.replay(r.runs, r.relay_used, r.work, r.metrics, by_report)
    assert by_report.state() == by_packet.state()
    assert by_report.log == by_packet.log
    assert r.ntunnels == len(by_packet.in_flags) == len(set(r.runs["key_id"].tolist()))
    return by_packet, by_report


@pytest.mark.parametrize("case", DIRECTED, ids=[c.name for c in DIRECTED])
def test_directed_case(case):
    by_packet, by_report = check(case.batch, case.plane)
    # the report never calls handleHostRoaming more often than the walk, and changes remotes as often
    assert by_report.roams == by_packet.roams
    assert by_report.denied <= by_packet.denied and by_report.suppressed <= by_packet.suppressed


@pytest.mark.parametrize("k", range(len(RANDOM)))
def test_random_batch(k):
    deny = RC.addr("10.9.0.2", 5001)
    check(RANDOM[k], lambda: M.ControlPlane(allow=lambda key, src: src != deny, remote={0: RC.addr("10.9.0.1", 5000)},
                                            last_roam={1: 999.0}, last_roam_remote={1: RC.addr("10.9.0.3", 5002)}))


def test_the_replay_saves_calls():
    """The point of the report: 70 000 packets cost the caller a few thousand roaming calls."""
    b = next(c for c in DIRECTED if c.name == "n_70000").batch
    r = report_host(b.pk, b.status, b.arena, b.frm, b.pkt_entry)
    assert r.metrics[L.METRIC_OPENED] > 60000 and len(r.runs) < r.metrics[L.METRIC_OPENED] // 20


def test_argument_errors():
    b = next(c for c in DIRECTED if c.name == "n_255").batch
    n = len(b)
    runs, used, work = (np.zeros(n * 40 + 8, np.uint8), np.zeros(n * 8 + 8, np.uint8), np.zeros(n * 8 + 8, np.uint8))
    metrics, counts = np.zeros(17, np.uint64), np.zeros(5, np.uint32)
    at = lambda a, k=0: C.c_void_p(a.ctypes.data + k)  # noqa: E731
    base = dict(pk=at(b.pk), st=at(b.status), n=n, arena=at(b.arena), alen=b.arena.nbytes, frm=at(b.frm), pe=at(b.pkt_entry),
                nfrom=len(b.frm), flags=0, runs=at(runs), used=at(used), work=at(work), metrics=at(metrics), counts=at(counts))
    call = lambda **o: L.lib().neb_rx_report_batch_host(*{**base, **o}.values())  # noqa: E731
    assert call() == L.OK and call(frm=None, pe=None, nfrom=0) == L.OK and call(pe=None) == L.OK
    assert call(flags=L.REPORT_RELAYED) == L.OK
    for over in (dict(pk=None), dict(st=None), dict(arena=None), dict(runs=None), dict(used=None), dict(work=None),
                 dict(metrics=None), dict(counts=None), dict(n=1 << 31), dict(flags=2), dict(flags=1 << 31),
                 dict(runs=at(runs, 4)), dict(metrics=at(metrics, 4)), dict(used=at(used, 2)), dict(work=at(work, 1)),
                 dict(counts=at(counts, 2)), dict(pk=at(b.pk.view(np.uint8), 2)), dict(st=at(b.status.view(np.uint8), 1)),
                 dict(frm=at(b.frm.view(np.uint8), 2)), dict(pe=at(b.pkt_entry.view(np.uint8), 2))):
        assert call(**over) == L.ERR_INVALID, over
    # 4-byte alignment is enough for everything but runs and metrics
    assert call(used=at(used, 4), work=at(work, 4), counts=at(counts, 4), metrics=at(metrics, 8), runs=at(runs, 8)) == L.OK
    # n == 0 needs no arrays and zeroes counts and metrics
    metrics[:], counts[:] = 7, 7
    assert call(n=0, pk=None, st=None, arena=None, runs=None, used=None, work=None) == L.OK
    assert not metrics[:16].any() and not counts[:4].any() and metrics[16] == 7 and counts[4] == 7


def test_arena_is_checked_before_anything_is_written():
    b = RC.Builder("entry")
    for _ in range(5):
        b.add(L.STATUS_OK, length=64)
    batch = b.batch()
    last = int(batch.pk["off"][-1]) + 64
    rc, outs, metrics, counts = run_raw(batch, arena_len=last)
    assert rc == L.OK and counts[0] == 1
    rc, outs, metrics, counts = run_raw(batch, arena_len=last - 1)
    assert rc == L.ERR_INVALID
    assert all((o == RC.FILL).all() for o in outs.values()) and (counts == 0xA5A5A5A5).all() and (metrics == 0xA5A5A5A5).all()
    for off, ln in ((1 << 63, 64), ((1 << 64) - 8, 16), (0, 0x7FFFFFFF), (batch.arena.nbytes - 15, 16)):
        batch.pk[2] = (off, ln, 7)
        assert run_raw(batch)[0] == L.ERR_INVALID, (off, ln)
    # a packet without a header is not read, wherever it claims to be
    batch.pk[2] = ((1 << 64) - 1, 15 | L.RX_OWN_SOURCE, 7)
    rc, outs, metrics, counts = run_raw(batch)
    assert rc == L.OK and metrics[L.METRIC_OPENED] == 5
