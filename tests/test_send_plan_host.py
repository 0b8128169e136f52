"""CPU: neb_tx_send_plan_host's ABI on exact-size numpy buffers: the argument errors, which write
nothing; outputs beyond nwires, niov and nentries untouched; the device form's argument checks, which
come before any device work."""
import ctypes as C

import numpy as np

import send_plan_cases as SC
import send_plan_ref as M
from nebula_amd import _lib as L

FILL = 0xA5


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(b, n=None, slack=0, **over):
    """The host form over the first n wires, the four outputs sized n + slack and filled with FILL."""
    wires, st, packets, via, remote = SC.arrays(b)
    n = len(wires) if n is None else n
    out = {"iov": np.full((n + slack) * 16, FILL, np.uint8), "entries": np.full((n + slack) * 16, FILL, np.uint8),
           "wire_entry": np.full((n + slack) * 4, FILL, np.uint8), "send_status": np.full((n + slack) * 4, FILL, np.uint8)}
    ni, ne = C.c_uint32(0xDEAD), C.c_uint32(0xBEEF)
    a = {"wires": _vp(wires), "wire_status": _vp(st), "nwires": n, "packets": _vp(packets), "npackets": len(packets),
         "via": _vp(via), "remote": _vp(remote), "ntunnels": len(remote), "socket_v4": int(b.socket_v4),
         "max_segments": b.max_segments, "chunk_packets": b.chunk_packets, "iov": _vp(out["iov"]), "niov": C.byref(ni),
         "entries": _vp(out["entries"]), "nentries": C.byref(ne), "wire_entry": _vp(out["wire_entry"]),
         "send_status": _vp(out["send_status"])}
    a.update(over)
    rc = L.lib().neb_tx_send_plan_host(*a.values())
    return rc, out, ni.value, ne.value


def _big():
    return SC.batch([(1200, SC.A)] * 5 + [(1200, SC.BAD6), (600, SC.B, SC.NS), (900, SC.B), (900, SC.B), (1, 99)])


def test_outputs_beyond_the_counts_are_untouched():
    b = _big()
    for n in (len(b.lens), 7, 0):
        sub = M.Batch(lens=b.lens[:n], packet=b.packet[:n], flags=b.flags[:n], status=b.status[:n], pkt_tunnel=b.pkt_tunnel,
                      remote=b.remote, via=b.via, out_off=b.out_off[:n])
        want = SC.plan_arrays(M.sequential(sub))
        rc, out, ni, ne = _call(b, n=n, slack=3)
        assert rc == L.OK and ni == len(want[0]) and ne == len(want[1])
        for name, w, item, cnt in (("iov", want[0], 16, ni), ("entries", want[1], 16, ne), ("wire_entry", want[2], 4, n),
                                   ("send_status", want[3], 4, n)):
            assert out[name][:cnt * item].tobytes() == w.tobytes(), name
            assert (out[name][cnt * item:] == FILL).all(), name


def test_exact_size_outputs():
    b = _big()
    rc, out, ni, ne = _call(b)
    want = SC.plan_arrays(M.sequential(b))
    assert rc == L.OK and (ni, ne) == (7, 2)
    assert out["wire_entry"].tobytes() == want[2].tobytes() and out["send_status"].tobytes() == want[3].tobytes()


def test_argument_errors_write_nothing():
    b = _big()
    for over in ({"max_segments": 1025}, {"wires": None}, {"wire_status": None}, {"packets": None}, {"remote": None},
                 {"iov": None}, {"entries": None}, {"wire_entry": None}, {"send_status": None}, {"niov": None},
                 {"nentries": None}):
        rc, out, ni, ne = _call(b, **over)
        assert rc == L.ERR_INVALID, over
        assert (ni, ne) == (0xDEAD, 0xBEEF) and all((v == FILL).all() for v in out.values()), over
    assert _call(b, max_segments=1024)[0] == L.OK
    assert _call(b, via=None)[0] == L.OK  # via may be NULL


def test_empty_batch_needs_no_arrays():
    ni, ne = C.c_uint32(9), C.c_uint32(9)
    rc = L.lib().neb_tx_send_plan_host(None, None, 0, None, 0, None, None, 0, 1, 63, 128, None, C.byref(ni), None, C.byref(ne),
                                       None, None)
    assert rc == L.OK and (ni.value, ne.value) == (0, 0)


def test_device_form_checks_arguments_before_any_device_work():
    z = np.zeros(64, np.uint8)
    p = _vp(z)
    lib = L.lib()
    # no engine; max_segments above 1024
    assert lib.neb_tx_send_plan(None, p, p, p, 1, p, 1, None, p, 1, 1, 63, 128, p, p, p, p, p, p, None) == L.ERR_INVALID
    assert lib.neb_tx_send_plan(None, p, p, p, 1, p, 1, None, p, 1, 1, 1025, 128, p, p, p, p, p, p, None) == L.ERR_INVALID
