"""CPU: neb_rx_recv_plan_host against the model (tests/recv_plan_ref.py) on every directed case and on
seeded random batches, through both inputs of the segment size, over FILL-initialised exact-size numpy
buffers: everything in [0, max_packets) and [0, nentries) as specified, padding included, nothing
beyond touched, the optional outputs left alone when NULL; the argument errors, which write nothing;
and the device form's argument checks, which come before any device work."""
import ctypes as C

import numpy as np
import pytest

import recv_plan_cases as RC
import recv_plan_ref as M
from nebula_amd import _lib as L

DIRECTED = RC.directed()


def _check(b, use_ctrl, slack, optional=True):
    p = M.listen_out(b, use_ctrl)
    rc, out, counts = RC.host_plan(b, use_ctrl, p.max_packets, slack, optional)
    assert rc == L.OK
    RC.compare(out, counts, RC.plan_arrays(p, len(b.entries)), slack, optional)


@pytest.mark.parametrize("case", DIRECTED, ids=[c.name for c in DIRECTED])
def test_directed_case(case):
    _check(case.batch, True, 3)
    _check(case.batch, False, 0)
    _check(case.batch, True, 2, optional=False)


def test_random_batches():
    for k, b in enumerate(RC.random_batches(99, 300)):
        _check(b, bool(k & 1), k % 3, optional=k % 5 != 0)


def _raw(over, nentries=2, max_packets=8, stride=64):
    """One call with valid arguments but for `over`; returns (rc, every output buffer, counts)."""
    en, ctrl = RC.arrays(RC.batch([RC.entry(3000, 1000) for _ in range(2)], ctrl_stride=64))
    ctrl = np.concatenate([ctrl, np.zeros(4096, np.uint8)])
    out = {name: np.full(64 * item, RC.FILL, np.uint8) for name, item in RC.OUT_ITEMS}
    counts = np.full(2, 0xDEADBEEF, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    a = {"entries": vp(en), "nentries": nentries, "ctrl": vp(ctrl), "ctrl_stride": stride, "socket_v4": 1, "pk": vp(out["pk"]),
         "src": vp(out["src"]), "pkt_entry": vp(out["pkt_entry"]), "max_packets": max_packets, "from": vp(out["from"]),
         "entry_first": vp(out["entry_first"]), "counts": vp(counts)}
    a.update(over)
    return L.lib().neb_rx_recv_plan_host(*a.values()), out, counts


def test_argument_errors_write_nothing():
    for over in ({"entries": None}, {"pk": None}, {"entry_first": None}, {"counts": None}, {"nentries": 1 << 31},
                 {"max_packets": 1 << 31}, {"max_packets": 0xFFFFFFFF}, {"ctrl_stride": 0}, {"ctrl_stride": 20},
                 {"ctrl_stride": 1032}):
        rc, out, counts = _raw(over)
        assert rc == L.ERR_INVALID, over
        assert counts.tolist() == [0xDEADBEEF] * 2 and all((v == RC.FILL).all() for v in out.values()), over
    assert _raw({})[0] == L.OK
    assert _raw({"ctrl_stride": 1024}, nentries=2)[0] == L.OK
    assert _raw({"ctrl": None, "ctrl_stride": 20})[0] == L.OK    # the stride counts only with control buffers
    assert _raw({"src": None, "pkt_entry": None, "from": None})[0] == L.OK
    rc, out, counts = _raw({"entries": None, "nentries": 0})      # no entries: d_entries may be NULL
    assert rc == L.OK and counts.tolist() == [0, 0]
    assert (out["pkt_entry"][:32].view(np.uint32) == L.RECV_NONE).all() and (out["pkt_entry"][32:] == RC.FILL).all()


def test_device_form_checks_arguments_before_any_device_work():
    z = np.zeros(64, np.uint64)
    p = z.ctypes.data_as(C.c_void_p)
    lib = L.lib()
    assert lib.neb_rx_recv_plan(None, p, 1, p, 64, 1, p, p, p, 4, p, p, p, None) == L.ERR_INVALID  # no engine
